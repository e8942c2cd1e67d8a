// The 16x16x32 kernel of the symmetric 3x3 convolution (conv3s.hip has the family's description and the 32x32x16 kernel): the
// Cout-128 forward on 4 x 32 patches — every forward 3x3 of the hourglass's 64 x 64 level — on v_mfma_f32_16x16x32_f16.
// Why (round 5): the chip holds a higher clock under the 4-pass MFMA (MI355X_MICROARCH "DVFS give-back"), an MFMA covers both K-steps
// of a pair, and the LDS image needs no padding (60 KB per workgroup instead of 80).  Same products, same (chunk, tap) order of the
// pairs as the 32x32x16 kernel; inside a pair the two steps are one 32-deep dot product, so the sums agree with that kernel's to fp32
// rounding, not bit for bit.  Measured (profiles/r05_ab_switches.txt box J, r05_pmc_issue_accounting.txt last section): forward 92-95
// us against 104-108 on the same boxes — 192 k cycles at 2.08 GHz against 205 k at 1.90 GHz, the matrix pipe busy for the same
// 54-58 % of them: the form buys clock.  In the hg2 / hg8 steps the difference stays inside the run-to-run spread.
//
// LDS.  An MFMA spans BOTH K-steps of a pair, a lane's 8 k-values are one 16-byte half of a pixel's (weight row's) 16-channel K-step,
// and the layouts keep the halves in planes of their own, 16 bytes per pixel / row, dense: the 16 lanes of a k-group read 16
// consecutive 16-byte slots and the four k-groups sit a multiple of 256 bytes apart -> every ds_read_b128 is conflict-free without
// padding
//   halo chunk buffer   [plane hi|lo][half][208 px][16 B]      x 2 buffers  (13 KB each against 19 KB)
//   ring slot           [plane hi|lo][k-group 0..3][128][16 B] x 3 slots    (16 KB against 20 KB; k-group = 2 (K-step of the pair) + half)
//   statistics scratch  [2][128][2] floats
//   BatchNorm vectors   [2][Cin] floats
// The weight pairs go global -> LDS directly (buffer_load_dwordx4 ... lds: a wave-instruction writes 64 lanes x 16 B = one k-group's
// 64 rows, contiguous in the layout above), three pairs ahead into the THREE-slot ring — no VGPR round trip (16 registers), no
// ds_write; the statistics scratch then has 2 KB of its own (no ring slot is ever free).
#include "conv3s_parts.h"

namespace {
constexpr int CO = 128, PW = 32;
constexpr int SUBPL = 208 * 16, APL = 2 * SUBPL, ABUF = 2 * APL;
constexpr int BPL = 4 * CO * 16, BSLOT = 2 * BPL;
constexpr int MF_LDS = 2 * ABUF + 3 * BSLOT + 2048 + 1024;
}

// PRO: the BatchNorm + ReLU prologue on the operand; RES1: one residual (conv3s's MODE 1, otherwise MODE 0)
template <bool PRO, bool RES1>
__global__ __launch_bounds__(256, 2) void conv3s_mf_kernel(ConvP p, int ntiles) {
    const int vstep = (int)gridDim.x;
    constexpr int WN = 2, WM = 2, TM = 2, TN = 2;
    typedef C3Patch<PW> T;
    constexpr int HW = T::HW, ITEMS = T::ITEMS;
    static_assert(T::HPX <= 204, "halo buffer");
    extern __shared__ __attribute__((aligned(16))) unsigned char c3_smem[];
    unsigned char* As = c3_smem;
    unsigned char* Bs = c3_smem + 2 * ABUF;
    float* RED = reinterpret_cast<float*>(Bs + 3 * BSLOT);              // the epilogue's statistics scratch [WM][CO][2]
    float* SS = reinterpret_cast<float*>(Bs + 3 * BSLOT + 2048);        // PRO: [2][Cin] BN scale / shift x operand scale

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
    const int ybytes = (int)((size_t)p.M * p.Cout * 4u);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res1 ? p.res1 : p.y), 0, ybytes, 0x00020000);
    const unsigned rowbytes = (unsigned)p.Cout * 4u;

    // ---- halo staging: item = tid + 256 j (< 816) -> halo pixel item >> 2, 4-channel quad item & 3
    const int kc = tid & 3;
    // `aok` (flags, c3_set_tile) belongs to the items being STORED, `aokn` to the tile whose offsets are in aoffs (they differ for a
    // few iterations around a tile change)
    unsigned aoffs[4], aok = 0, aokn = 0;
    auto set_tile = [&](const int vv) { return c3_set_tile<PW, false>(p, ntiles, tws, ths, vv, tid, kc, aoffs, aokn); };
    // Halo staging, ROLLING (conv3s.hip): ONE item is fetched and ONE stored per iteration, each item four iterations after its
    // fetch, through a ring of four register sets (item j <-> set j)
    c3_u32x4 ra[4];
    const float lo_valid = p.in_relu ? 0.f : -__builtin_inff();
    c3_fill_vectors<PRO, false>(p, SS, sa, tid);
    auto load1 = [&](c3_u32x4& a, const int c, const int j) { a = __builtin_amdgcn_raw_buffer_load_b128(xr, aoffs[j], c * 64, 0); };
    // item j of chunk c: transform, split, two 8-byte LDS stores; okb = the aok bits of the tile the item belongs to.  Whole items
    // are decided at compile time; the threads beyond the end of the LAST, partial item run the same instructions on zeros (their
    // loads were out of range) and park the result in pixels 204 .. 207 of a half-plane (never read).
    auto store1 = [&](const c3_u32x4 a, const int buf, const int c, const int j, const unsigned okb) {
        if (256 * j >= ITEMS) return;                           // (compile time: j is a constant after unrolling)
        const bool active = (256 * j + 255 < ITEMS) || (tid + 256 * j < ITEMS);
        uint2 q1, q2;
        c3_item<PRO, false>(p, SS, a, a, c, j, okb, kc, lo_valid, sa, yr, aoffs[j], q1, q2);    // (no second stream, no dL/dy store)
        unsigned char* dst = As + buf * ABUF +
            ((kc >> 1) * SUBPL + (active ? (tid >> 2) + 64 * j : 204 + ((tid >> 2) & 3)) * 16 + (kc & 1) * 8);
        *reinterpret_cast<uint2*>(dst) = q1;
        *reinterpret_cast<uint2*>(dst + APL) = q2;
    };
    auto ld = [&](const int c, const int j) { load1(ra[j], c, j); };
    auto st = [&](const int buf, const int c, const int j) { store1(ra[j], buf, c, j, aok); };

    // ---- weight stream by LDS-DMA: pair gp = K-steps 2 gp, 2 gp + 1 = 2 x [CO][16] fp16 per plane, contiguous.  Wave w copies unit
    // blocks 4 w .. 4 w + 3 of a pair (16 blocks of 64 rows x 16 B): block = plane (w >> 1), k-group 2 (w & 1) + (j >> 1), row half
    // j & 1.  LDS destination = M0 (wave-uniform) + lane x 16; global source = lane x 32 (VGPR) + a scalar offset (the stream keeps a
    // weight row's two halves side by side: [K-step][row][2 x 16 B]).  hipcc does not count these loads: the waits are placed by
    // hand, by the guide's rule — the wait before a barrier, the reads after it.
    int gp = 0;                                 // the pair the NEXT dmaB fetches
    const unsigned wplane = (unsigned)((size_t)p.wq_stride * 2u);
    const c3_i32x4 wrs = {(int)(unsigned)(size_t)p.wq, (int)((unsigned)((size_t)p.wq >> 32) & 0xffffu),
                          (int)(((size_t)p.wq_stride + (size_t)p.Cout * p.K) * 2u), 0x00020000};
    const unsigned dma_voff = (unsigned)lane * 32u;
    const unsigned dma_lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)Bs
                              + (unsigned)((wave >> 1) * BPL + (wave & 1) * 2 * (CO * 16));
    const unsigned dma_g0 = (unsigned)(wave >> 1) * wplane + (unsigned)(wave & 1) * 4096u;
    auto dmaB = [&](const unsigned slot) {
        // the four pieces: LDS + 1024 j, stream + {0, 2048, 16, 2064}; M0 is written in the statement that uses it and restored (the
        // compiler owns it); an SALU instruction between every write of M0 and the load that reads it
        const unsigned so = (unsigned)gp * (unsigned)(CO * 64) + dma_g0, la = dma_lds0 + slot;
        unsigned keep, t;
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %2\n\t"
                     "s_add_u32 %1, %3, 0x800\n\t"
                     "buffer_load_dwordx4 %4, %5, %3 offen lds\n\t"
                     "s_add_u32 m0, m0, 0x400\n\t"
                     "s_nop 0\n\t"
                     "buffer_load_dwordx4 %4, %5, %1 offen lds\n\t"
                     "s_add_u32 m0, m0, 0x400\n\t"
                     "s_add_u32 %1, %3, 16\n\t"
                     "buffer_load_dwordx4 %4, %5, %1 offen lds\n\t"
                     "s_add_u32 m0, m0, 0x400\n\t"
                     "s_add_u32 %1, %3, 0x810\n\t"
                     "buffer_load_dwordx4 %4, %5, %1 offen lds\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep), "=&s"(t)
                     : "s"(la), "s"(so), "v"(dma_voff), "s"(wrs)
                     : "scc");
        gp = gp + 1 == npairs ? 0 : gp + 1;
    };

    // ---- fragments: the wave tile (2 patch rows x 64 channels) as 4 x 4 blocks of 16 pixels x 16 channels.  Fragment sets of
    // 2 blocks x 2 planes: X / W = the activation rows of block rows 0-1 / 2-3, Y / Z = the weight rows of block columns 0-1 / 2-3.
    // A lane's k-groups 0-1 belong to K-step 2 it (tap, chunk buffer of that step), 2-3 to step 2 it + 1: a per-lane select
    // between two constants.  Quarter order X Y, X Z | barrier | W Y, W Z: each set is read once per pair (16 reads),
    // Z and W (this pair) in the first half, X and Y of the NEXT pair in the second — X is dead after the first half, Y after the
    // third quarter — so all reads of pair it fall between the barriers of it - 1 and it, the epoch the ring and the staging
    // schedule keep that pair's slot and chunk buffers stable for
    typedef f16x8 FSet[2][2];
    FSet X, Y, Z, W;
    c3_f32x4 acc16[4][4];
    // (one address register per operand: block r of the wave tile is a compile-time offset away)
    const bool khi = (lane & 32) != 0;
    const unsigned a16base = (unsigned)(((wm * TM * HW + (lane & 15)) * 16) + ((lane >> 4) & 1) * SUBPL);
    const unsigned b16base = (unsigned)((lane >> 4) * (CO * 16) + (wn * 64 + (lane & 15)) * 16);
    auto a16off = [&](const int r) { return ((r >> 1) * HW + 16 * (r & 1)) * 16; };
    auto b16off = [&](const int r) { return r * 256; };
    // local K-steps s0, s0 + 1 of a chunk pair (0..17; 18 = step 0 of the next pair): chunk buffer (s / 9) & 1, tap s % 9
    auto ldA = [&](FSet& S, const int rbp, const int s0) {
        const int t0 = s0 % 9, t1 = (s0 + 1) % 9;
        const unsigned c0 = (unsigned)(((s0 / 9) & 1) * ABUF + ((t0 / 3) * HW + t0 % 3) * 16);
        const unsigned c1 = (unsigned)((((s0 + 1) / 9) & 1) * ABUF + ((t1 / 3) * HW + t1 % 3) * 16);
        const unsigned char* src = As + (a16base + (khi ? c1 : c0));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) S[i][pl] = *reinterpret_cast<const f16x8*>(src + (a16off(2 * rbp + i) + pl * APL));
    };
    auto ldB = [&](FSet& S, const int cbp, const unsigned slot) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) S[i][pl] = *reinterpret_cast<const f16x8*>(Bs + (slot + b16base) + (b16off(2 * cbp + i) + pl * BPL));
    };
    auto mmq = [&](const FSet& A, const FSet& B, const int rbp, const int cbp) {
        // (term-major: the three MFMAs of a block are four MFMAs apart — a dependent 4-pass MFMA issued back to back waits for the
        // result of the one before; each block still sums lo x hi, hi x lo, hi x hi in this order)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    c3_f32x4& c = acc16[2 * rbp + i][2 * cbp + j];
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[i][t == 0], B[j][t == 1], c, 0, 0, 0);
                }
    };
    // result element e (0..15) of the 32-pixel x 32-channel block (a, b) of the wave tile, for the epilogue
    auto accv = [&](const int a, const int b, const int e) { return acc16[2 * a + (e >> 3)][2 * b + ((e >> 2) & 1)][e & 3]; };
    auto accz = [&](const int a, const int b, const int e) { acc16[2 * a + (e >> 3)][2 * b + ((e >> 2) & 1)][e & 3] = 0.f; };
    auto zero = [&]() {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) accz(a, b, e);
    };

    const float am2lo = p.tail.amax_relu ? 0.f : -__builtin_inff();
    float am = 0.f, am2 = 0.f;

    // ---- epilogue.  A 32 x 32 block of the wave tile is four 16 x 16 results (a lane: 16 channels lane & 15 of pixels
    // 4 (lane >> 4) + r — a store would write four 64-byte runs, and two instructions share every 128-byte line).
    // v_permlane16_swap of the two column blocks' registers (odd 16-lane rows of one <-> even rows of the other) turns them into the
    // 32 x 32 shape: element e = pixel 16 (e>>3) + 4 ((e>>2)&1) + (e&3) + 8 lh of patch row wm TM + a, channel lr of column tile
    // wn TN + b — two full lines per store, one channel column per lane.  red: statistics scratch [WM][CO][2]
    auto epilogue = [&](float* red, const int m0) {
        constexpr int NT = TM * TN;
        float rbuf[2][16];
        auto tile_off = [&](const int i) {       // i = b * TM + a
            const int a = i % TM, b = i / TM;
            return (unsigned)((m0 + (wm * TM + a) * p.W + 8 * lh) * p.Cout + (wn * TN + b) * 32 + lr) * 4u;
        };
        auto reg_off = [&](const int e) { return (unsigned)((e & 3) + 4 * ((e >> 2) & 1) + 16 * (e >> 3)) * rowbytes; };
        auto loadres = [&](float (&r)[16], const int i) {
            if (!RES1) return;
            const unsigned o0 = tile_off(i);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const unsigned so = reg_off(e);
                r[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r1r, o0, so, 0));
            }
        };
        auto loadcol = [&](const int b) { return c3_loadcol<false>(p, (wn * TN + b) * 32 + lr); };
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
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                c3_f32x4& c0 = acc16[2 * a + (q >> 2)][2 * b], & c1 = acc16[2 * a + (q >> 2)][2 * b + 1];
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(c0[q & 3]), __float_as_uint(c1[q & 3]), false, false);
                c0[q & 3] = __uint_as_float(sw[0]);
                c1[q & 3] = __uint_as_float(sw[1]);
            }
            const float (&r)[16] = rbuf[i & 1];
            const unsigned o0 = tile_off(i);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const unsigned so = reg_off(e);
                float val = accv(a, b, e) * osc;
                val += col.cb;
                if (RES1) val += r[e];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), yr, o0, so, 0);
                am = fmaxf(am, fabsf(val));
                if (p.tail.amax_bn) am2 = fmaxf(am2, fabsf(fmaxf(fmaf(val, col.sc, col.sh), am2lo)));
                s1 += val;
                s2 = fmaf(val, val, s2);
                accz(a, b, e);
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
    int v = (int)blockIdx.x;
    int m0 = set_tile(v), m0n = 0;
    aok = aokn;
    dmaB(0); dmaB(BSLOT); dmaB(2 * BSLOT);      // pairs 0, 1, 2
    {
        // chunk 0 whole and item 0 of chunk 1 through temporaries (one round trip); the next items of chunk 1 stay in flight in
        // the ring, as the loop's schedule expects them at it = 0
        c3_u32x4 t[5];
#pragma unroll
        for (int j = 0; j < 4; ++j) load1(t[j], 0, j);
        load1(t[4], 1, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) store1(t[j], 0, 0, j, aok);
        store1(t[4], 1, 1, 0, aok);
        ld(1, 1); ld(1, 2); ld(1, 3);
    }
    asm volatile("s_waitcnt vmcnt(0)");
    unsigned bcur = 0, bnxt = BSLOT, bnn = 2 * BSLOT;
    __syncthreads();
    ldA(X, 0, 0);
    ldB(Y, 0, bcur);
    zero();

    for (; v < ntiles; v += vstep) {
        for (int c2 = 0; c2 < nchunks; c2 += 2) {
#pragma unroll
            for (int it = 0; it < 9; ++it) {
                // first half: the MFMAs of the pair's quarters X Y, X Z carry the reads of Z and W
                __builtin_amdgcn_sched_barrier(0);
                ldB(Z, 1, bcur);
                ldA(W, 1, 2 * it);
                mmq(X, Y, 0, 0);
                mmq(X, Z, 0, 1);
                // the eight fragment reads behind the first eight MFMAs (Z is due at the 13th)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                // (the LDS-write and vector-memory groups below date from a weight ring fed through registers and match nothing
                // since the ring is filled by DMA; the sequence still shapes the order of the remaining MFMAs — without it the
                // compiler emits another schedule, which nobody has measured — so it stays as it was timed)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // the pair whose fragments are read behind this barrier was asked for two iterations ago: younger, and allowed
                // to be in flight, are the halo fetch issued right behind it, the four pieces of the previous iteration's pair and
                // that iteration's fetch (iteration 8 of a chunk pair fetches nothing).  The first two iterations of a tile
                // have nothing to wait for (prologue / the wait before the epilogue retired everything) — and must not wait:
                // the epilogue's stores are in the same queue
                if (it >= 2 || c2 != 0) {
                    if (it <= 1) asm volatile("s_waitcnt vmcnt(5)");
                    else asm volatile("s_waitcnt vmcnt(6)");
                }
                __syncthreads();                // the other slots / chunk buffer are written; this slot is read
                // second half: the MFMAs of the quarters W Y, W Z carry the reads of X and Y of the next pair and the halo staging
                ldA(X, 0, 2 * it + 2);
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
                    // this pair's slot has been read for the last time (Z, before the barrier): the pair three ahead goes
                    // there.  Between the item's store and the next item's fetch: hipcc's own count in front of the store does not
                    // know the four pieces — `vmcnt(3)` for the three younger fetches then means "all but the youngest three
                    // operations", i.e. it also retires every fetch older than the last piece; with the fetch BEHIND the pieces that
                    // is the fetch of two iterations ago (a lead of two left of the four), with the fetch in front of them it
                    // would be the previous iteration's
                    dmaB(bcur);
                    if (it == 0 && last) m0n = set_tile(v + vstep);
                    if (it <= 3) ld(cn0, it);
                    else if (it <= 7) ld(cn1, it - 4);
                }
                mmq(W, Y, 1, 0);
                ldB(Y, 0, bnxt);
                mmq(W, Z, 1, 1);
                {
                    // 24 MFMAs: the reads of X (next pair) behind MFMAs 1-4, of Y behind 13-16 — Y is this pair's operand through
                    // the 12th, and the next pair's first MFMA wants it 8 MFMAs after the last read —, the item's VALU spread over
                    // the first 20, its fetch and stores at the end
                    // (the item's BatchNorm vectors are LDS reads too — NSS of them: asked for right behind X, or the item's VALU
                    // waits for them in one clump)
                    constexpr int NSS = PRO ? 2 : 0, VS = NSS ? 8 : 0, VPG = PRO ? 4 : 1;
#pragma unroll
                    for (int i = 0; i < 24; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (i < 4 || (i >= 12 && i < 16) || (it != 3 && i >= 4 && i < 4 + NSS)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        if (it != 3 && i >= VS && i < 22) __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);
                        if (it != 3 && i == 22) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                        if (it != 3 && i == 23) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                { const unsigned tsw = bcur; bcur = bnxt; bnxt = bnn; bnn = tsw; }
            }
        }

        // (every piece in flight is retired here — behind the epilogue its stores would stand in the queue before them)
        asm volatile("s_waitcnt vmcnt(0)");
        epilogue(RED, m0);
        if (p.stats) c3_tile_stats<CO, WM>(p, RED, v, ntiles, 0, tid);
        m0 = m0n;
    }
    if (p.tail.amax) amax_commit(am, p.tail.amax);
    if (p.tail.amax_bn) amax_commit(am2, p.tail.amax_bn, 1);
    asm volatile("s_waitcnt vmcnt(0)");         // (nothing may still be writing this workgroup's LDS when it ends)
}

template <bool PRO, bool RES1>
static void c3_mf_launch_k(const ConvP& p, hipStream_t st, int grid, int ntiles) {
    DSNT_SET_MAX_LDS((conv3s_mf_kernel<PRO, RES1>), MF_LDS);
    DSNT_LAUNCH((conv3s_mf_kernel<PRO, RES1>), dim3(grid), dim3(256), MF_LDS, st, p, ntiles);
}

void dsnt_conv3s_mf_launch(const ConvP& p, bool pro, hipStream_t st, int grid, int ntiles) {
    if (pro) {
        if (p.res1) c3_mf_launch_k<true, true>(p, st, grid, ntiles);
        else c3_mf_launch_k<true, false>(p, st, grid, ntiles);
    } else if (p.res1) c3_mf_launch_k<false, true>(p, st, grid, ntiles);
    else c3_mf_launch_k<false, false>(p, st, grid, ntiles);
}
