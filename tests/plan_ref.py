"""The host-side plans of the fp16x3 streaming convolution kernels, restated in plain Python with the CU count as a parameter:
what csrc/{wgrad1,wgrad3,fwd1,bwd1,gemm1,conv3s,stem4}.hip launch their kernels with (slabs, stages per workgroup, iterations,
column chunks, rows per slab); and, at the end, the dispatch of the fp32 family of csrc/conv_f32.hip (conv_f32: no CU count enters it) and of the tiled split-precision kernels of
csrc/conv_split6.hip (conv_split).  tests/test_plan_edges_cpu.py asks it which edges a case hits; tests/test_plan_edges_gpu.py first
holds it to what the C ABI reports on the real device.  A geometry the plan refuses gives None.

Cases are (N, H, W, Cin, Cout); `share` is the DSNT_CONV_SHARE_CHIP / DSNT_WGRAD_SHARE_CHIP form of the launch.  wgrad1 and wgrad3
size their launches for 256 CUs whatever the device has (a constant in the source), so `cus` does not enter them."""

LIMIT = 1 << 31             # every tensor is addressed with 32-bit byte offsets


def _fits(rows, *channels):
    return all(rows * c * 4 < LIMIT for c in channels)


def wgrad1(case, cus=256, share=False):
    N, H, W, Cin, Cout = case
    M = N * H * W
    if M < 16384 or M % 16 or not _fits(M, Cin, Cout):
        return None
    if Cin % 256 == 0 and Cout % 128 == 0 and Cout % 256 != 0:
        ck, cn = 256, 128
    elif Cin % 128 == 0 and Cout % 256 == 0:
        ck, cn = 128, 256
    elif Cin % 128 == 0 and Cout % 128 == 0:
        ck, cn = 128, 128
    elif Cin % 64 == 0 and Cout % 128 == 0:
        ck, cn = 64, 128
    elif Cin % 128 == 0 and Cout % 64 == 0:
        ck, cn = 128, 64
    elif Cin % 64 == 0 and Cout % 64 == 0:
        ck, cn = 64, 64
    else:
        return None
    kchunks, nchunks = Cin // ck, Cout // cn
    sp = min(max((128 if share else 256) // (kchunks * nchunks), 1), M // 128)
    rows = (-(-M // sp) + 15) // 16 * 16
    nsplits = -(-M // rows)
    last = M - (nsplits - 1) * rows
    return dict(ck=ck, cn=cn, kchunks=kchunks, nchunks=nchunks, rows_per_split=rows, nsplits=nsplits, last_rows=last,
                nstages=rows // 16, last_stages=last // 16)


F1_CFGS = [(256, 128, 8, 1), (128, 256, 8, 1), (128, 128, 8, 1), (64, 64, 4, 1), (64, 128, 8, 1), (256, 256, 8, 2)]   # Cin, Cout, waves, chunks
B1_CFGS = [(256, 128, 8, 1), (128, 256, 8, 1), (128, 128, 8, 1), (64, 64, 4, 1), (64, 128, 4, 1), (256, 256, 8, 2)]
FWD1_DS_PAIRS = [(64, 128), (128, 256)]


def _stages(case, cus, share, cfgs, min_rows):
    N, H, W, Cin, Cout = case
    M = N * H * W
    if M % 32 or M < min_rows or not _fits(M, Cin, Cout):
        return None
    cfg = [c for c in cfgs if c[:2] == (Cin, Cout)]
    if not cfg:
        return None
    _, _, waves, chunks = cfg[0]
    nstages = M // 32
    nwg = cus * (2 if waves == 4 else 1) // chunks
    if share:
        nwg = max(nwg // 2, 1)
    if chunks > 1 and nwg // 8 * 8 > 0:
        nwg = nwg // 8 * 8
    nwg = min(nwg, nstages)
    spw = -(-nstages // nwg)
    nwg = -(-nstages // spw)
    return dict(nstages=nstages, spw=spw, nwg=nwg, last=nstages - (nwg - 1) * spw, chunks=chunks, waves=waves)


def fwd1(case, cus=256, share=False):
    return _stages(case, cus, share, F1_CFGS, 4096)


def bwd1(case, cus=256, share=False):
    return _stages(case, cus, share, B1_CFGS, 16384)


def gemm1(case, cus=256, share=False):
    N, H, W, K, Cout = case
    M = N * H * W
    if M < 65536 or not _fits(M, K, Cout):
        return None
    if K == 128:
        ntw = 8 if Cout % 256 == 0 else 4 if Cout % 128 == 0 else 2 if Cout % 64 == 0 else 0
    elif K == 256:
        ntw = 4 if Cout % 128 == 0 else 0
    elif K == 64:
        ntw = 4 if Cout % 128 == 0 else 2 if Cout % 64 == 0 else 0
    else:
        return None
    rows_it = 8 * (8 // ntw) * 32 if ntw else 0
    if not ntw or M % rows_it:
        return None
    niter, chunks = M // rows_it, Cout // (32 * ntw)
    grid = cus // chunks
    if share:
        grid = max(grid // 2, 1)
    grid = min(max(grid, 1), niter)
    return dict(ntw=ntw, rows_it=rows_it, niter=niter, chunks=chunks, grid=grid)


def wgrad3(case, cus=256, share=0):
    """share: 0 the whole chip, 1 DSNT_WGRAD_SHARE_CHIP, 2 with DSNT_WGRAD_NARROW on top."""
    N, H, W, Cin, Cout = case
    if Cin % 64 or Cout % 64:
        return None
    WS = 64 if W >= 64 else W
    if WS not in (16, 32, 64) or W % WS or not _fits(N * H * W, Cin, Cout):
        return None
    cfg = 0 if Cout % 128 == 0 else 1
    strips, kchunks, nchunks = W // WS, Cin // 64, Cout // (64 if cfg else 128)
    per = kchunks * nchunks * strips * N
    small = bool(share) and cfg == 0                # four-wave workgroups of 32 input channels: twice the workgroups per slab
    want = 128 if small else 256
    if share == 2:
        want //= 2
    rps = H
    while per * (H // rps) < want and rps % 2 == 0 and (rps // 2) * (WS // 16) >= 32:
        rps //= 2
    hsplits = H // rps
    nslabs = N * hsplits * strips
    return dict(cfg=2 if small else cfg, WS=WS, strips=strips, kchunks=kchunks, nchunks=nchunks, rps=rps, hsplits=hsplits,
                nslabs=nslabs, blocks=kchunks * nchunks * nslabs * (2 if small else 1))


def conv3s(case, cus=256, mode=0, share=False):
    """mode: 0 / 1 forward (without / with a residual), 3 the BatchNorm-backward epilogue, 4 the folded BatchNorm backward.
    form: bit 0 two 64-column halves per patch, bit 1 the 16x16x32 MFMA form, bit 2 8 x 16 patches (dsnt_conv_fwd_stream_form)."""
    N, H, W, Cin, Cout = case
    w32 = H % 4 == 0 and W % 32 == 0
    if not (w32 or (H % 8 == 0 and W % 16 == 0)) or Cin % 32 or Cin > 128 or Cout not in (64, 128):
        return None
    if mode not in (0, 1, 3, 4) or not _fits(N * H * W, Cin, Cout):
        return None
    ntiles = N * (H // (4 if w32 else 8)) * (W // (32 if w32 else 16))
    if Cout == 128 and mode != 4 and ntiles <= 128:
        form = 1 | (0 if w32 else 4)
    elif not w32:
        form = 4
    else:
        form = 2 if Cout == 128 and mode in (0, 1) else 0
    grid = min(cus + cus // 2 if share else 2 * cus, ntiles)
    if form & 1:
        grid = 2 * ntiles
    return dict(form=form, ntiles=ntiles, grid=grid, patch_rows=H // (8 if form & 4 else 4), kpairs=9 * Cin // 32)


def stem4(case, cus=256):
    """case = (N, Ho, Wo) of the 4x4 / stride 1 / pad 1 convolution of the [N][Ho + 1][Wo + 1][16] space-to-depth image."""
    N, Ho, Wo = case
    if Ho % 4 or Wo % 32 or not _fits(N * Ho * Wo, 64) or not _fits(N * (Ho + 1) * (Wo + 1), 16):
        return None
    ntiles = N * (Ho // 4) * (Wo // 32)
    return dict(tiles=ntiles, tile_rows=Ho // 4, tile_cols=Wo // 32, grid=min(2 * cus, ntiles), wgrad_grid=min(cus, ntiles))


def route(case, k, wgrad, stem=False):
    """dsnt_conv_f16x3_route for a stride-1 convolution with a k x k filter (stem: case = (N, Ho, Wo))."""
    if stem:
        return (1 if wgrad else 0) if stem4(case) else None
    if wgrad:
        if k == 3 and wgrad3(case):
            return 2
        return 3 if k == 1 and wgrad1(case) else 0
    if k == 1 and gemm1(case):
        return 1
    N, H, W, Cin, Cout = case
    return 2 if k == 3 and H % 8 == 0 and W % 16 == 0 and Cin % 32 == 0 else 0


KSPLIT_ROWS = 2048          # csrc/conv_f32.hip ksplit_rows(): output rows up to which the K-split kernel replaces the 32 x 128 tiling
KSPLIT_PRO_CIN = 4096       # ... with a BatchNorm prologue: both vectors live in the kernel's 8448 floats of LDS


def conv_f32(case, pro=False, amax=False):
    """The fp32 family of csrc/conv_f32.hip (pick_cfg, the K-split conditions of conv_fwd_impl, `fast` of launch_fwd) for
    case = (N, H, W, Cin, Cout, k, stride, pad, dil).  pro: the launch has in_scale / in_shift; amax: its dsnt_out_bounds asks for
    amax or amax_bn (the K-split epilogue has neither).  `bm` is what dsnt_conv_fwd_bm reports: the rows per statistics tile.
    kernel: ksplit16 / ksplit8 (chunk width; `chunks` = the set of chunks per wave) or t128x128 / t128x64 / t128x32 / t32x128
    (`fast`: the wave-uniform-tap loader; `nsteps` K-steps of 32, `ktail`: the last one is partial)."""
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    if min(N, H, W, Cin, Cout, k, stride, dil, Ho, Wo) <= 0 or pad < 0 or Cin % 4 or Cout % 4:
        return None
    M, K = N * Ho * Wo, k * k * Cin
    if N * H * W * Cin >= LIMIT or M * Cout >= LIMIT:
        return None
    BM, BN = 128, 32 if Cout <= 32 else 64 if Cout <= 64 else 128
    if -(-M // BM) * -(-Cout // BN) < 256 and Cout >= 128:      # few rows: more workgroups for less register blocking
        BM, BN = 32, 128
    fits = N * H * W * Cin * 4 < LIMIT and Cout * K * 4 < LIMIT       # 32-bit byte offsets of the buffer loads
    out = dict(bm=BM, M=M, K=K, ragged_m=M % BM != 0)
    if BM == 32 and M <= KSPLIT_ROWS and Cin % 8 == 0 and fits and not amax and (not pro or Cin <= KSPLIT_PRO_CIN):
        cw = 16 if Cin % 16 == 0 else 8
        nch = K // cw
        out.update(kernel='ksplit%d' % cw, chunks={(w + 1) * nch // 8 - w * nch // 8 for w in range(8)},
                   mtiles=-(-M // 32), ntiles=-(-Cout // 32), ragged_n=Cout % 32 != 0)
        return out
    out.update(kernel='t%dx%d' % (BM, BN), fast=Cin % 32 == 0 and k * k * (BM // 32) <= 64 and fits, nsteps=-(-K // 32),
               ktail=K % 32 != 0, mtiles=-(-M // BM), ntiles=-(-Cout // BN), ragged_n=Cout % BN != 0)
    return out


FWD6_BN64_ROWS = 8192       # csrc/conv_split6.hip FWD6_BN64_ROWS_DEFAULT: output rows up to which Cout % 64 == 0 runs on 64-wide tiles.
                            # A PREMISE: DSNT_X_FWD6_BN64_ROWS moves it, no test sets that, and the ABI does not show the tile width
PITCH6 = 24                 # csrc/conv_split.h: bf16 / fp16 elements per LDS row of 16


def conv_split(case, path='bf16x6'):
    """conv_fwd6_impl of csrc/conv_split6.hip for case = (N, H, W, Cin, Cout, R, S, stride, pad, dil) below the streaming kernels
    (gemm1 takes 1x1 convolutions of 65536 rows and more on the fp16x3 path: refused here).  kernel: 'halo' (conv3x3_halo_ok, the
    8 x 16 patch kernel, TN = bn / 64) or 'gemm' (the implicit GEMM on 128 x bn tiles); mtiles = the statistics rows; nsteps =
    K / 16 K-steps ('gemm') or nchunks = Cin / 16 ('halo'); lds = the bytes of LDS the launch asks for on `path` (three bf16 or two
    fp16 planes; the epilogue's C tile where that is larger); trips = passes of the 256 loader threads over the BatchNorm vectors
    of a prologue ('gemm': they live behind the tiles in LDS; the halo kernel reads them from memory)."""
    N, H, W, Cin, Cout, R, S, stride, pad, dil = case
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    if min(N, H, W, Cin, Cout, R, S, stride, dil, Ho, Wo) <= 0 or pad < 0 or Cin % 16 or Cout % 4 or R * S > 16:
        return None
    M, K = N * Ho * Wo, R * S * Cin
    if N * H * W * Cin * 4 >= LIMIT or M * Cout >= LIMIT or 3 * Cout * K * 2 >= LIMIT:
        return None
    if path == 'f16x3' and R == S == 1 and stride == 1 and pad == 0 and gemm1((N, H, W, Cin, Cout)):
        return None
    halo = (R, S, stride, pad, dil) == (3, 3, 1, 1, 1) and H % 8 == 0 and W % 16 == 0 and Cin % 32 == 0
    bn = 64 if Cout <= 64 or (M <= FWD6_BN64_ROWS and Cout % 64 == 0 and not halo) else 128
    npl = 2 if path == 'f16x3' else 3
    out = dict(kernel='halo' if halo else 'gemm', bn=bn, M=M, K=K, mtiles=-(-M // 128), ntiles=-(-Cout // bn), ragged_m=M % 128 != 0,
               ragged_n=Cout % bn != 0)
    epi = 128 * (bn + 4) * 4
    if halo:
        out.update(nchunks=Cin // 16, trips=0, lds=max(((2 if npl == 2 else 1) * npl * 192 + 2 * npl * bn) * PITCH6 * 2, epi))
    else:
        out.update(nsteps=K // 16, trips=-(-Cin // 256), lds=max(2 * npl * (128 + bn) * PITCH6 * 2 + 2 * Cin * 4, epi))
    return out
