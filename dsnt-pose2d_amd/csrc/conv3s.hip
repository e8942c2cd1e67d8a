// 3x3 / stride 1 / pad 1 convolutions of the full-resolution levels (hourglass.py:22-23: conv2 of every Bottleneck, forward
// and as data gradients) on the fp16 matrix cores, fp16x3 split — the SYMMETRIC successor of conv3x3_bf16x6_kernel (conv_split6.hip).
//
// What that kernel lost (profiles/r02_timeline_halo.txt, r02_pmc_issue_accounting.txt): its four loader waves share the
// SIMDs with the four MFMA waves, lose the issue arbitration against them and arrive last at 80 % of the per-K-step
// barriers (803 of 1993 cycles per step are barrier wait on the MFMA waves); prologue and epilogue (LDS transposition of
// the 128 x 128 result) are another 18 k cycles per tile with the matrix pipe idle.  Here:
//   * four waves, ALL alike: every wave copies its share of the weights and of the input halo between its own MFMAs
//     (an MFMA holds the vector issue port for 8 of its 32 cycles — the staging work of a step fits beside them);
//   * a tile is a 4 x 32 patch (8 x 16 where the image is 16 pixels wide) of output pixels x all Cout (64 / 128) columns; the
//     (4+2) x (32+2) input halo of a 16-channel chunk is transformed (BatchNorm + ReLU, operand scale) and split ONCE into LDS, double-buffered;
//   * the weights come pre-split in STREAM order ([chunk][tap][Cout][16]: dsnt_f16_prep_weights, row flag): a K-step
//     pair is one contiguous 16 KB block, copied with coalesced 16-byte loads one pair ahead into a two-slot ring;
//   * ONE barrier per pair of K-steps (24 MFMAs per wave), placed between the two steps: the fragments of the step
//     after the barrier are read while the MFMAs of the step before it run, so no fragment read is exposed;
//   * workgroups are persistent: the weight stream wraps around and the next tile's first halo chunk is staged by the
//     regular schedule of the last chunk pair — a tile has no prologue; the epilogue works from the MFMA result layout
//     (a register = 2 pixels x 32 consecutive channels = two 128-byte runs; no LDS transposition), residual loads
//     software-pipelined over the wave's tiles (as gemm1.hip).
// Same K order (16-channel chunk, tap) and MFMA order as conv3x3_bf16x6_kernel<.., F16>: the convolution sums of this kernel are
// bit-identical to that kernel's; the per-tile column statistics are summed in another order.
// Two kernels: this file's, on v_mfma_f32_32x32x16_f16 — every data gradient, Cout 64, the 8 x 16 patches and the column split —
// and conv3s_mf.hip's, on v_mfma_f32_16x16x32_f16 — the Cout-128 forward on 4 x 32 patches; c3_form below chooses.  What does not
// depend on the MFMA form (tile -> halo offsets, the transform of a halo item, column vectors, statistics) is in conv3s_parts.h.
// Contract: conv_fwd_bf16x6_kernel<..., F16> minus the second residual (dsnt_conv3s_ok).
// Measured (DESIGN.md "round 3", profiles/r03_pmc_issue_accounting.txt): 3x3 128->128 @64x64, batch 32: 129 -> 104 us on one box
// (matrix pipe 53 %, 1.15 PFLOP/s of fp16 MFMA at the ~1.9 GHz this load holds), -0.42 ms per hg2 step.  Built on the same pieces,
// bit-identical, and dropped: an 8-wave ping-pong form (two groups one phase apart, 101-110 us, but one 124 KB workgroup per CU
// starves the other lanes: +0.07 ms per step), deeper halo prefetch (108 us), a start-up stagger of the CU's second workgroup (+-0).
#include "conv3s_parts.h"
#include <stdlib.h>

#ifndef C3_SPLIT_TILES_DEFAULT
#define C3_SPLIT_TILES_DEFAULT 128
#endif

// LDS of the 32x32x16 kernel (device and host): padded rows, every ds_read_b128 conflict-free
//   halo chunk buffer  [plane hi|lo][204 px][48 B]   x 2 buffers
//   ring slot          [plane hi|lo][CO][80 B]       x 2 slots
//   BatchNorm vectors  [2 or 3][Cin] floats
#define C3_HPX 204                          /* halo pixels of a 4 x 32 patch (6 x 34); an 8 x 16 patch needs 10 x 18 = 180 */
#define C3_AP 48                            /* bytes per halo pixel and plane: 16 fp16 + 16 (conflict-free ds_read_b128) */
#define C3_APL (C3_HPX * C3_AP)
#define C3_ABUF (2 * C3_APL)
#define C3_BP 80                            /* bytes per weight row and plane of a slot: 2 x 16 fp16 + 16 */
static constexpr int c3_lds(const int co, const int mode) { return 2 * C3_ABUF + 2 * (2 * co * C3_BP) + (mode == 4 ? 1536 : 1024); }

// MODE: 0 no residual, 1 res1, 3 the BatchNorm-backward epilogue of a data-gradient launch (res1 = the BatchNorm input x),
// 4 = 3 with the BatchNorm backward of the layer BEHIND folded into the operand load (round 5): the A operand is not dL/dy but
//     dL/dz (ReLU-masked, reduced) and y, two streams, and every element is formed as  dy = scale (dz - c0 - (y - mean) invstd c1)
//     = P dz + R y + S  while it is staged (the separate dsnt_bn_act_bwd_apply pass in front of every 3x3 data gradient is gone);
//     the 128 pixels of the patch itself (not the halo ring: each pixel of the image is interior to exactly one patch) are also
//     written to p.ap_out — the materialised dL/dy the weight gradient reads afterwards.  The affine form carries the
//     conditioning of a scale / shift BatchNorm forward (eps |mean| / std), like `fmaf(x, scale, shift)` everywhere else.
// PW: the patch is 128 / PW rows of PW pixels — 4 x 32 (W % 32 == 0), or 8 x 16 for the 16-pixel-wide levels (a 32-pixel MFMA
// tile then spans two patch rows: a few two-way LDS bank conflicts on the activation fragments, immaterial at that size)
// SP (round 5): a 128-column convolution with too few patches to fill the chip (the 16 x 16 and 32 x 32 levels of the 8-stack net at batch
// 16: 32 / 128 patches on 512 slots) runs as TWO 64-column halves per patch — CO = 64 code, the weight stream and every column index
// offset by 64 x (blockIdx & 1): twice the workgroups, half the MFMAs per K-step and workgroup; both stage the same halo.  Every
// output is the same sum in the same order as in the unsplit kernel (bit-identical).
template <int CO, bool PRO, int MODE, int PW, bool SP>
__global__ __launch_bounds__(256, 2) void conv3s_kernel(ConvP p, int ntiles) {
    static_assert(!SP || (CO == 64 && MODE != 4), "column split: 64-column code, one-stream modes");
    constexpr int COG = SP ? 2 * CO : CO;          // columns of a weight row block in the stream
    const int choff = SP ? CO * (int)(blockIdx.x & 1) : 0;
    const int vstep = SP ? (int)(gridDim.x >> 1) : (int)gridDim.x;
    constexpr int WN = CO / 64, WM = 4 / WN, TM = 4 / WM, TN = 2;
    typedef C3Patch<PW> T;
    constexpr int HW = T::HW, ITEMS = T::ITEMS;
    static_assert(T::HPX <= C3_HPX, "halo buffer");
    constexpr int APL = C3_APL, ABUF = C3_ABUF, BPL = CO * C3_BP, BSLOT = 2 * BPL;
    constexpr bool APPLY = MODE == 4, BNB = MODE >= 3;
    static_assert(!(APPLY && PRO), "the folded BatchNorm backward replaces the prologue");
    constexpr int NJB = CO / 32;                // 16-byte weight units per thread and K-step pair
    constexpr int UPP = 4 * CO;                 // units per plane and pair
    extern __shared__ __attribute__((aligned(16))) unsigned char c3_smem[];
    unsigned char* As = c3_smem;                // [2 chunk buffers][2 planes][204 px][48]
    unsigned char* Bs = c3_smem + 2 * ABUF;     // [2 slots][2 planes][CO][80]
    float* SS = reinterpret_cast<float*>(Bs + 2 * BSLOT);       // PRO: [2][Cin] BN scale / shift x operand scale; APPLY: [3][Cin] P, R, S

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int nchunks = p.Cin >> 4;             // even
    const int npairs = nchunks * 9 / 2;
    const int tws = p.W / PW, ths = p.H / T::PH;
    const float sa = pow2_scale(bound64(p.a_bound)), sw = pow2_scale(bound64(p.w_bound));
    const float osc = 1.f / (sa * sw);

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x), 0, (int)((size_t)p.M * p.Cin * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(p.wq), 0, (int)(((size_t)p.wq_stride + (size_t)p.Cout * p.K) * 2u), 0x00020000);
    const int ybytes = (int)((size_t)p.M * p.Cout * 4u);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res1 ? p.res1 : p.y), 0, ybytes, 0x00020000);
    const unsigned rowbytes = (unsigned)p.Cout * 4u;
    const int xbytes = (int)((size_t)p.M * p.Cin * 4u);
    const __amdgpu_buffer_rsrc_t x2r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(APPLY ? p.ap_y : p.x), 0, xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t dor = __builtin_amdgcn_make_buffer_rsrc(APPLY ? p.ap_out : p.y, 0, APPLY ? xbytes : ybytes, 0x00020000);

    // ---- halo staging: item = tid + 256 j (< 816) -> halo pixel item >> 2, 4-channel quad item & 3
    const int kc = tid & 3;
    // `aok` (flags, c3_set_tile) belongs to the items being STORED, `aokn` to the tile whose offsets are in aoffs (they differ for a
    // few iterations around a tile change)
    unsigned aoffs[4], aok = 0, aokn = 0;
    auto set_tile = [&](const int vv) { return c3_set_tile<PW, APPLY>(p, ntiles, tws, ths, vv, tid, kc, aoffs, aokn); };
    // Halo staging, ROLLING (round 5): a chunk is 4 items per thread; instead of fetching a whole chunk at once and storing it two
    // iterations later, ONE item is fetched and ONE stored per iteration, each item LEAD iterations after its fetch, through a ring
    // of NSLOT register sets (item j <-> set j % NSLOT).  One stream: LEAD 4, four sets — 16 registers; two streams (MODE 4): LEAD 2,
    // two sets of two (with both streams fetched a chunk at a time the kernel spilled: 256 VGPRs + 68 B of scratch).  What it buys
    // is issue overlap, and only together with the branch-free item (c3_item): an item's ~50 VALU instructions (transform + split)
    // are spread over the 12 MFMAs of its step by the scheduling groups (against fetching and storing a chunk at a time: 1 % faster
    // at 64 x 64, 5 % at 32 x 32, and -0.10 ms per hg2 step: profiles/r05_ab_switches.txt box E).
    constexpr int NSLOT = APPLY ? 2 : 4, LEAD = APPLY ? 2 : 4;
    c3_u32x4 ra[NSLOT], ra2[APPLY ? NSLOT : 1];
    const float lo_valid = p.in_relu ? 0.f : -__builtin_inff();
    c3_fill_vectors<PRO, APPLY>(p, SS, sa, tid);
    auto load1 = [&](c3_u32x4& a, c3_u32x4& b, const int c, const int j) {
        a = __builtin_amdgcn_raw_buffer_load_b128(xr, aoffs[j], c * 64, 0);
        if (APPLY) b = __builtin_amdgcn_raw_buffer_load_b128(x2r, aoffs[j], c * 64, 0);
    };
    // item j of chunk c: transform, split, two 8-byte LDS stores; okb = the aok bits of the tile the item belongs to.  Whole items
    // are decided at compile time; the threads beyond the end of the LAST, partial item run the same instructions on zeros (their
    // loads were out of range) and park the result in the pad bytes (32 .. 47 of a pixel's 48, never read) of a pixel row.
    // (APPLY: the offsets of a tile are stable from its first fetch to its last store: set_tile comes after the last store of the
    // previous tile's items)
    auto store1 = [&](const c3_u32x4 a, const c3_u32x4 b, const int buf, const int c, const int j, const unsigned okb) {
        if (256 * j >= ITEMS) return;                           // (compile time: j is a constant after unrolling)
        const bool active = (256 * j + 255 < ITEMS) || (tid + 256 * j < ITEMS);
        uint2 q1, q2;
        c3_item<PRO, APPLY>(p, SS, a, b, c, j, okb, kc, lo_valid, sa, dor, aoffs[j], q1, q2);
        unsigned char* dst = As + buf * ABUF + (active ? ((tid >> 2) + 64 * j) * C3_AP + kc * 8 : (tid >> 2) * C3_AP + 32 + (kc & 1) * 8);
        *reinterpret_cast<uint2*>(dst) = q1;
        *reinterpret_cast<uint2*>(dst + APL) = q2;
    };
    // the ring: item j lives in register set j % NSLOT
    auto ld = [&](const int c, const int j) { load1(ra[j % NSLOT], ra2[APPLY ? j % NSLOT : 0], c, j); };
    auto st = [&](const int buf, const int c, const int j) { store1(ra[j % NSLOT], ra2[APPLY ? j % NSLOT : 0], buf, c, j, aok); };

    // ---- weight stream: pair gp = K-steps 2 gp, 2 gp + 1 = 2 x [CO][16] fp16 per plane, contiguous
    unsigned bvoff[NJB], blds[NJB];
#pragma unroll
    for (int j = 0; j < NJB; ++j) {
        const int u = tid + 256 * j, pl = u / UPP, uu = u % UPP;
        bvoff[j] = (unsigned)((size_t)pl * p.wq_stride * 2u) +
                   (SP ? (unsigned)((uu / (2 * CO)) * (COG * 32) + choff * 32 + (uu % (2 * CO)) * 16) : (unsigned)uu * 16u);
        // (stream order of a pair and plane: [K-step][CO][2 halves of 16 bytes])
        blds[j] = (unsigned)(pl * BPL + ((uu >> 1) % CO) * C3_BP + (uu / (2 * CO)) * 32 + (uu & 1) * 16);
    }
    c3_u32x4 rb[NJB];
    int gp = 0;                                 // the pair the NEXT gloadB fetches
    auto gloadB = [&]() {
        const unsigned so = (unsigned)gp * (unsigned)(COG * 64);
#pragma unroll
        for (int j = 0; j < NJB; ++j) rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, bvoff[j], so, 0);
        gp = gp + 1 == npairs ? 0 : gp + 1;
    };
    auto storeB = [&](const unsigned slot) {
#pragma unroll
        for (int j = 0; j < NJB; ++j) *reinterpret_cast<c3_u32x4*>(Bs + (slot + blds[j])) = rb[j];
    };

    // ---- fragments
    struct Frag { f16x8 a[TM][2], b[TN][2]; };
    unsigned aoff[TM], boff[TN];
#pragma unroll
    for (int a = 0; a < TM; ++a) {
        const int mt = wm * TM + a;              // 32-pixel tile of the patch: one patch row (PW 32) or two (PW 16)
        const int prow = PW == 32 ? mt : 2 * mt + (lr >> 4), pcol = lr & (PW - 1);
        aoff[a] = (unsigned)((prow * HW + pcol) * C3_AP + 16 * lh);
    }
#pragma unroll
    for (int b = 0; b < TN; ++b) boff[b] = (unsigned)(((wn * TN + b) * 32 + lr) * C3_BP + 16 * lh);
    // local K-step s of a chunk pair (0..17; 18 = step 0 of the next pair): chunk buffer (s / 9) & 1, tap s % 9
    auto rd = [&](Frag& F, const int s, const unsigned slot) {
        const int t = s % 9, buf = (s / 9) & 1;
        const int toff = buf * ABUF + ((t / 3) * HW + (t % 3)) * C3_AP;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
                F.a[a][pl] = *reinterpret_cast<const f16x8*>(As + aoff[a] + toff + pl * APL);
#pragma unroll
            for (int b = 0; b < TN; ++b)
                F.b[b][pl] = *reinterpret_cast<const f16x8*>(Bs + slot + boff[b] + pl * BPL + (s & 1) * 32);
        }
    };
    f32x16 acc[TM][TN];
    auto mm = [&](const Frag& F) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.a[a][1], F.b[b][0], acc[a][b], 0, 0, 0);
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.a[a][0], F.b[b][1], acc[a][b], 0, 0, 0);
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.a[a][0], F.b[b][0], acc[a][b], 0, 0, 0);
            }
    };
    auto zero = [&]() {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    };

    const float am2lo = p.tail.amax_relu ? 0.f : -__builtin_inff();
    float am = 0.f, am2 = 0.f;

    // ---- epilogue from the C layout: register e of a 32 x 32 tile = pixels (e&3) + 8 (e>>2) + 4 lh of patch row wm TM + a, channel
    // lr of column tile wn TN + b.  red: statistics scratch [WM][CO][2]
    auto epilogue = [&](float* red, const int m0) {
        constexpr int NT = TM * TN;
        float rbuf[2][16];
        auto tile_off = [&](const int i) {       // i = b * TM + a
            const int a = i % TM, b = i / TM;
            return (unsigned)((m0 + (wm * TM + a) * (PW == 32 ? 1 : 2) * p.W + 4 * lh) * p.Cout + choff + (wn * TN + b) * 32 + lr) * 4u;
        };
        // register e -> pixel (e&3) + 8 (e>>2) + 4 lh of the 32-pixel tile; PW 16: pixels 16.. are the next patch row
        auto reg_off = [&](const int e) {
            return PW == 32 ? (unsigned)((e & 3) + 8 * (e >> 2)) * rowbytes
                            : (unsigned)((e >> 3) * p.W + (e & 3) + 8 * ((e >> 2) & 1)) * rowbytes;
        };
        auto loadres = [&](float (&r)[16], const int i) {
            if (MODE == 0) return;
            const unsigned o0 = tile_off(i);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const unsigned so = reg_off(e);
                r[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r1r, o0, so, 0));
            }
        };
        auto loadcol = [&](const int b) { return c3_loadcol<BNB>(p, choff + (wn * TN + b) * 32 + lr); };
        C3Col col = loadcol(0), coln = col;
        loadres(rbuf[0], 0);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int a = i % TM, b = i / TM;
            if (i + 1 < NT) {
                loadres(rbuf[(i + 1) & 1], i + 1);
                if ((i + 1) % TM == 0) coln = loadcol((i + 1) / TM);
            }
            __builtin_amdgcn_sched_barrier(0);
            const float (&r)[16] = rbuf[i & 1];
            const unsigned o0 = tile_off(i);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const unsigned so = reg_off(e);
                float val = acc[a][b][e] * osc;
                if (BNB) {
                    // val = dL/d relu(bn(x)); r = x: mask by the ReLU, accumulate the BatchNorm-backward sums
                    const float xv = r[e];
                    if (p.bnb_relu && fmaf(xv, col.sc, col.sh) <= 0.f) val = 0.f;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), yr, o0, so, 0);
                    s1 += val;
                    s2 = fmaf(val, (xv - col.mu) * col.is, s2);
                    am = fmaxf(am, fabsf(val));          // max |dz| (p.tail.amax: the bound of a folded BatchNorm backward)
                } else {
                    val += col.cb;
                    if (MODE >= 1) val += r[e];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), yr, o0, so, 0);
                    am = fmaxf(am, fabsf(val));
                    if (p.tail.amax_bn) am2 = fmaxf(am2, fabsf(fmaxf(fmaf(val, col.sc, col.sh), am2lo)));
                    s1 += val;
                    s2 = fmaf(val, val, s2);
                }
                acc[a][b][e] = 0.f;
            }
            if (a == TM - 1) {
                if (p.stats) {
                    s1 += __shfl_xor(s1, 32, 64);
                    s2 += __shfl_xor(s2, 32, 64);
                    if (lh == 0) {
                        red[(wm * CO + (wn * TN + b) * 32 + lr) * 2 + 0] = s1;
                        red[(wm * CO + (wn * TN + b) * 32 + lr) * 2 + 1] = s2;
                    }
                }
                s1 = 0.f; s2 = 0.f;
                col = coln;
            }
        }
    };
    // ---- prologue of the workgroup's FIRST tile
    int v = SP ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;
    int m0 = set_tile(v), m0n = 0;
    aok = aokn;
    gloadB();
    {
        // chunk 0 whole and item 0 of chunk 1 through temporaries (one round trip); the next items of chunk 1 stay in flight in
        // the ring, as the loop's schedule expects them at it = 0
        c3_u32x4 t[5], t2[APPLY ? 5 : 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) load1(t[j], t2[APPLY ? j : 0], 0, j);
        load1(t[4], t2[APPLY ? 4 : 0], 1, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) store1(t[j], t2[APPLY ? j : 0], 0, 0, j, aok);
        store1(t[4], t2[APPLY ? 4 : 0], 1, 1, 0, aok);
        if (LEAD == 4) { ld(1, 1); ld(1, 2); ld(1, 3); }
        else { ld(1, 1); ld(1, 2); }
    }
    storeB(0);
    gloadB();                                   // pair 1 travels
    unsigned bcur = 0, bnxt = BSLOT;
    __syncthreads();
    Frag F0, F1;
    rd(F0, 0, bcur);
    zero();

    for (; v < ntiles; v += vstep) {
        for (int c2 = 0; c2 < nchunks; c2 += 2) {
#pragma unroll
            for (int it = 0; it < 9; ++it) {
                // first half: the MFMAs of step 2 it carry the fragment reads of step 2 it + 1, the copy of the pair after this
                // one into the other slot (its last readers passed the previous barrier) and the fetch of the one after that
                __builtin_amdgcn_sched_barrier(0);
                rd(F1, 2 * it + 1, bcur);
                storeB(bnxt);
                gloadB();
                mm(F0);
#pragma unroll
                for (int i = 0; i < 4 * TM; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
#pragma unroll
                for (int i = 0; i < NJB; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();                // the other slot / chunk buffer is written; this slot is read
                // second half: the MFMAs of step 2 it + 1 carry the fragment reads of step 2 it + 2 and the halo staging
                rd(F0, 2 * it + 2, bnxt);
                {
                    // buffer 1 (the odd chunk c2 + 1: read from step 9, last read at step 17 of the previous pair) takes its items at
                    // it = 8 of the previous pair and it = 0, 1, 2; buffer 0 (the next even chunk, or chunk 0 of the next tile: last
                    // read at step 8) at it = 4 .. 7; the store comes first, the fetch of a later item re-uses its registers
                    const bool last = c2 + 2 >= nchunks;
                    const int cn0 = last ? 0 : c2 + 2, cn1 = last ? 1 : c2 + 3;
                    if (it <= 2) st(1, c2 + 1, it + 1);
                    else if (it >= 4 && it <= 7) st(0, cn0, it - 4);
                    else if (it == 8) st(1, cn1, 0);
                    if (it == 3 && last) aok = aokn;                  // from it = 4 on the stored items are the next tile's
                    if (LEAD == 4) {
                        if (it == 0 && last) m0n = set_tile(v + vstep);
                        if (it <= 3) ld(cn0, it);
                        else if (it <= 7) ld(cn1, it - 4);
                    } else {
                        if (it == 0) ld(c2 + 1, 3);
                        if (it == 2 && last) m0n = set_tile(v + vstep);
                        if (it >= 2 && it <= 5) ld(cn0, it - 2);
                        else if (it >= 6) ld(cn1, it - 6);
                    }
                }
                mm(F1);
                {
                    // every MFMA of the step carries a fragment read (the first eight) and a few of the item's ~50 VALU instructions
                    // (transform + split: left in one clump they run with the matrix pipe idle on BOTH waves of the SIMD, which
                    // reach this point together); the item's fetch and its two LDS stores behind the last MFMAs
                    constexpr int VPG = APPLY ? 6 : (PRO ? 5 : 4);
#pragma unroll
                    for (int i = 0; i < 4 * TM; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        if (it != 3) __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, APPLY ? 2 : 1, 0);
                    if (it != 3) {
                        __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);
                        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (APPLY) __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                { const unsigned tsw = bcur; bcur = bnxt; bnxt = tsw; }
            }
        }

        float* red = reinterpret_cast<float*>(Bs + bnxt);      // `bnxt` (the slot just consumed) is free: statistics scratch [WM][CO][2]
        epilogue(red, m0);
        if (p.stats) c3_tile_stats<CO, WM>(p, red, v, ntiles, choff, tid);
        m0 = m0n;
    }
    if (p.tail.amax) amax_commit(am, p.tail.amax);
    if (p.tail.amax_bn) amax_commit(am2, p.tail.amax_bn, 1);
}

static int c3_enabled = -1;

bool dsnt_conv3s_geom_ok(const dsnt_conv_geom* g) {
    if (c3_enabled < 0) {
        c3_enabled = dsnt_kernel_off("conv3s") ? 0 : 1;
    }
    if (!c3_enabled || !g) return false;
    if (!(g->R == 3 && g->S == 3 && g->stride == 1 && g->pad == 1 && g->dil == 1 && g->Ho == g->H && g->Wo == g->W)) return false;
    if (!((g->H % 4 == 0 && g->W % 32 == 0) || (g->H % 8 == 0 && g->W % 16 == 0)) || g->Cin % 32 != 0 || g->Cin > 128) return false;
    if (g->Cout != 64 && g->Cout != 128) return false;
    const size_t M = (size_t)g->N * g->H * g->W;
    if (M * g->Cin * 4u >= (1ull << 31) || M * g->Cout * 4u >= (1ull << 31)) return false;
    return true;
}

bool dsnt_conv3s_ok(const ConvP& p) {
    dsnt_conv_geom g;
    memset(&g, 0, sizeof(g));
    g.N = p.N; g.H = p.H; g.W = p.W; g.Cin = p.Cin; g.Ho = p.Ho; g.Wo = p.Wo; g.Cout = p.Cout;
    g.R = p.R; g.S = p.S; g.stride = p.stride; g.pad = p.pad; g.dil = p.dil;
    if (!dsnt_conv3s_geom_ok(&g)) return false;
    if (!p.a_bound || !p.w_bound || !p.wq) return false;
    if (p.res2) return false;
    if (p.bnb_scale && p.in_scale) return false;
    if (p.ap_y && !(p.bnb_scale && p.ap_scale && p.ap_mean && p.ap_invstd && p.ap_coef && p.ap_out && !p.res2)) return false;
    return true;
}

// column split (SP) up to this many patches: DSNT_X_C3_SPLIT_TILES, A/B
static int c3_split_tiles() {
    static int m = -1;
    if (m < 0) { const char* e = getenv("DSNT_X_C3_SPLIT_TILES"); m = e ? atoi(e) : C3_SPLIT_TILES_DEFAULT; }
    return m;
}

// the kernel form a launch takes — the ONE place that decides it (the launcher below and dsnt_conv3s_form, which lets a test ask
// what ran): bit 0 column split (SP: two 64-column halves per patch), bit 1 the 16x16x32 kernel (MF), bit 2 8 x 16 patches.
// MF is the Cout-128 forward on 4 x 32 patches (alone, batch 32, 64 x 64: 97-99 us against 103-108 on the 32x32x16 kernel); the data
// gradients stay here (DESIGN_HISTORY.md "conv3s: the retired 16x16x32 data gradients").
static int c3_form(int cout, int mode, int N, int H, int W) {
    const bool w32 = W % 32 == 0 && H % 4 == 0;
    if (cout == 128 && mode != 4) {
        const int ntiles = N * (H / (w32 ? 4 : 8)) * (W / (w32 ? 32 : 16));
        if (ntiles <= c3_split_tiles()) return 1 | (w32 ? 0 : 4);
    }
    if (!w32) return 4;
    return cout == 128 && mode <= 1 ? 2 : 0;
}

// persistent workgroups over the patches of the launch
static int c3_grid(int ntiles, bool share, bool sp) {
    const int cus = dsnt_device_cus();
    int grid = 2 * cus;                         // two workgroups per CU (LDS)
    // DSNT_CONV_SHARE_CHIP: a launch on a side lane.  Two of these workgroups take a CU's whole LDS for the life of the launch,
    // and the dependency chain's small kernels on the other streams then wait for a slot (a bn_finalize of 8 workgroups: 63 us
    // instead of 6).  3/2 workgroups per CU: -0.08 ms per hg2 step (256 / 384 / 448 workgroups measured alike; once the side
    // lane's 1x1 kernel yields half of the CUs — gemm1.hip — this one's share no longer matters: 128 .. 512 workgroups within 0.03 ms).
    if (share) grid = cus + cus / 2;
    if (grid > ntiles) grid = ntiles;
    if (sp) grid = 2 * ntiles;                  // (only asked for when that is at most a slot per workgroup)
    return grid;
}

template <int CO, bool PRO, int MODE, int PW, bool SP>
static void c3_launch_k(const ConvP& p, hipStream_t st, bool share) {
    constexpr int lds = c3_lds(CO, MODE);
    DSNT_SET_MAX_LDS((conv3s_kernel<CO, PRO, MODE, PW, SP>), lds);
    const int ntiles = p.N * (p.H / (128 / PW)) * (p.W / PW);
    DSNT_LAUNCH((conv3s_kernel<CO, PRO, MODE, PW, SP>), dim3(c3_grid(ntiles, share, SP)), dim3(256), lds, st, p, ntiles);
}

template <int CO, bool PRO, int MODE>
static void c3_launch_m(const ConvP& p, hipStream_t st, bool share, int form) {
    if constexpr (CO == 128 && MODE != 4) {
        if (form & 1) {
            if (form & 4) return c3_launch_k<64, PRO, MODE, 16, true>(p, st, share);
            return c3_launch_k<64, PRO, MODE, 32, true>(p, st, share);
        }
    }
    if (form & 4) return c3_launch_k<CO, PRO, MODE, 16, false>(p, st, share);
    // (the Cout-128 forward on 4 x 32 patches is never here: split or on the 16x16x32 kernel)
    if constexpr (!(CO == 128 && MODE <= 1)) c3_launch_k<CO, PRO, MODE, 32, false>(p, st, share);
}

template <int CO>
static void c3_launch(const ConvP& p, bool pro, hipStream_t st, bool share, int mode, int form) {
    if (mode == 4) c3_launch_m<CO, false, 4>(p, st, share, form);
    else if (mode == 3) c3_launch_m<CO, false, 3>(p, st, share, form);
    else if (pro) {
        if (mode == 1) c3_launch_m<CO, true, 1>(p, st, share, form);
        else c3_launch_m<CO, true, 0>(p, st, share, form);
    } else if (mode == 1) c3_launch_m<CO, false, 1>(p, st, share, form);
    else c3_launch_m<CO, false, 0>(p, st, share, form);
}

void dsnt_conv3s_launch(const ConvP& p, bool pro, hipStream_t st, bool share) {
    const int mode = p.bnb_scale ? (p.ap_y ? 4 : 3) : (p.res1 ? 1 : 0);
    const int form = c3_form(p.Cout, mode, p.N, p.H, p.W);
    if (form & 2) {
        const int ntiles = p.N * (p.H / 4) * (p.W / 32);
        return dsnt_conv3s_mf_launch(p, pro, st, c3_grid(ntiles, share, false), ntiles);
    }
    if (p.Cout == 128) c3_launch<128>(p, pro, st, share, mode, form);
    else c3_launch<64>(p, pro, st, share, mode, form);
}

int dsnt_conv3s_form_of(const dsnt_conv_geom* g, int mode) {
    if (!dsnt_conv3s_geom_ok(g) || mode < 0 || mode > 4 || mode == 2) return -1;
    return c3_form(g->Cout, mode, g->N, g->H, g->W);
}
