// Forward / data-gradient convolutions on the bf16 and fp16 matrix cores in split precision (bf16x6 / fp16x3: conv_split.h):
// the implicit GEMM, the 3x3 LDS halo-tile kernel, and the dispatch of the dsnt_conv_fwd_bf16x6* / _f16x3* entry points
// into them, conv3s.hip and gemm1.hip.  Same contract as the fp32 kernels of conv_f32.hip.
#include "conv_epilogue.h"
#include "gemm1.h"
#include "conv3s.h"
#include "wgrad.h"
#include <string.h>
#include <stdlib.h>

template <int WM, int WN, int TM, int TN, bool PRO, bool F16 = false, int DA = 4>
__global__ __launch_bounds__(512, 2) void conv_fwd_bf16x6_kernel(ConvP p) {
    constexpr int NPL = F16 ? 2 : 3;            // operand planes (fp16x3: two fp16 planes, three MFMAs)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int APASS = BM / 64;             // loader: 64 rows x 4 float4 chunks per pass
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* A6 = reinterpret_cast<__bf16*>(smem);          // [2][NPL][BM][PITCH6]
    __bf16* B6 = A6 + 2 * NPL * BM * PITCH6;               // [2][NPL][BN][PITCH6]
    float* SS = reinterpret_cast<float*>(B6 + 2 * NPL * BN * PITCH6);   // [2][Cin]: BN scale / shift of the A operand

    int tile;
    xcd_remap(blockIdx.x, p.mtiles * p.ntiles, tile);
    const int ntile = tile % p.ntiles, mtile = tile / p.ntiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nsteps = p.K / BK6;
    const int lr = lane & 31, lh = lane >> 5;
    const int cw = wave & 3;
    const int wm = cw / WN, wn = cw % WN;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    if (wave >= 4) {
        // ------------------------------------------------------------------ loader waves
        const int ltid = tid - 256;
        // 16 consecutive lanes store 4 float4-chunks of rows {r, r+2, r+4, r+6}: with the 48-byte row
        // pitch those 16 ds_write_b64 hit 16 distinct 8-byte bank groups (rows r..r+3 would 2-way conflict)
        const int kc = ltid & 3;
        const int lrow = ((ltid >> 5) << 3) + (((ltid >> 2) & 3) << 1) + ((ltid >> 4) & 1);
        const int HoWo = p.Ho * p.Wo;
        const int RS = p.R * p.S;
        unsigned apix[APASS];
        unsigned vmask = 0;                          // bit tap*APASS + i
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            const int m = mtile * BM + lrow + 64 * i;
            const bool vm = m < p.M;
            const int mm = vm ? m : 0;
            const int n = mm / HoWo, rem = mm - n * HoWo;
            const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
            const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
            apix[i] = (unsigned)(((n * p.H + ih0) * p.W + iw0) * p.Cin + kc * 4) * 4u;
            for (int t = 0; t < RS; ++t) {
                const int r = t / p.S, s_ = t - r * p.S;
                const int ih = ih0 + r * p.dil, iw = iw0 + s_ * p.dil;
                if (vm && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) vmask |= 1u << (t * APASS + i);
            }
        }
        // weights: 16-byte chunk `ltid` of each plane's [BN][16] slice: row = ltid>>1, half = ltid&1
        const int bhalf = ltid & 1;     // same idea for the 16-byte weight stores (8-lane groups)
        const int brow = ((ltid >> 4) << 3) + (((ltid >> 1) & 3) << 1) + ((ltid >> 3) & 1);
        const int bn = ntile * BN + brow;
        const bool bvalid = brow < BN && bn < p.Cout;
        unsigned bpix[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            bpix[j] = bvalid ? (unsigned)((size_t)j * p.wq_stride + (size_t)bn * p.K + bhalf * 8) * 2u : 0xF0000000u;
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.x), 0, (int)((size_t)p.N * p.H * p.W * p.Cin * 4u), 0x00020000);
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<unsigned short*>(p.wq), 0, (int)(((size_t)(NPL - 1) * p.wq_stride + (size_t)p.Cout * p.K) * 2u), 0x00020000);
        // fp16x3: operand scale (a power of two) from the bound the producer left in device memory
        const float sa = F16 ? pow2_scale(bound64(p.a_bound)) : 1.f;
        // The A operand is what this kernel waits for: with K = 128 ... 256 a tile is 8 ... 16 K-steps, each a fresh
        // 8 KB slice of activations from HBM, and the chip-wide bytes in flight bound the bandwidth (Little's law: 512
        // resident workgroups x 2 stages x 8 KB = 8 MB gave 3.6 TB/s at ~2.2 us loaded latency).  DA register stages
        // keep DA slices per workgroup in flight; the weights (L2 hits) stay on two stages; the BatchNorm scale / shift
        // vectors live in LDS (copied once, pre-multiplied by the fp16x3 operand scale) instead of riding in every stage.
        struct AStage { u32x4 ra[APASS]; };
        struct BStage { u32x4 rb[NPL]; };
        AStage SA[DA];
        BStage SB[2];
        const float lo_valid = p.in_relu ? 0.f : -__builtin_inff();
        const int last = nsteps - 1;
        // K-step bookkeeping without divisions: the loads (A: DA steps ahead, B: two ahead) and the stores walk the
        // K-steps in order, so each keeps running scalars (channel base, filter tap) advanced branch-free and frozen
        // at the last step (the tail re-loads / re-stores it: never read, or into the idle buffer).  `kb / Cin` and
        // `tap / S` per call were ~100 instructions of emulated integer division per step on the waves the MFMA
        // waves wait for.
        struct Walk { int step, cb, r, s_; };
        Walk wa = {0, 0, 0, 0}, ws = {0, 0, 0, 0};
        int wb_step = 0;
        auto advance = [&](Walk& w) {
            const int adv = w.step < last ? 1 : 0;
            w.step += adv;
            w.cb += adv * BK6;
            const int wrap = w.cb >= p.Cin ? 1 : 0;
            w.cb = wrap ? 0 : w.cb;
            w.s_ += wrap;
            const int wrap2 = w.s_ == p.S ? 1 : 0;
            w.s_ = wrap2 ? 0 : w.s_;
            w.r += wrap2;
        };
        auto gloadA = [&](AStage& st) {
            const unsigned toff = (unsigned)(((wa.r * p.dil) * p.W + wa.s_ * p.dil) * p.Cin + wa.cb) * 4u;
#pragma unroll
            for (int i = 0; i < APASS; ++i)
                st.ra[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, apix[i] + toff, 0, 0);
            advance(wa);
        };
        auto gloadB = [&](BStage& st) {
            const unsigned koff = (unsigned)(wb_step * BK6) * 2u;
#pragma unroll
            for (int j = 0; j < NPL; ++j)
                st.rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, bpix[j] + koff, 0, 0);
            wb_step += wb_step < last ? 1 : 0;
        };
        auto lstore = [&](const AStage& sa_, const BStage& sb_, int buf) {
            const int cb = ws.cb;
            const unsigned okm = vmask >> ((ws.r * p.S + ws.s_) * APASS);
            advance(ws);
            float4 sc, sh;
            if (PRO) {
                sc = *reinterpret_cast<const float4*>(SS + cb + kc * 4);
                sh = *reinterpret_cast<const float4*>(SS + p.Cin + cb + kc * 4);
            }
#pragma unroll
            for (int i = 0; i < APASS; ++i) {
                float4 v = make_float4(__uint_as_float(sa_.ra[i].x), __uint_as_float(sa_.ra[i].y),
                                       __uint_as_float(sa_.ra[i].z), __uint_as_float(sa_.ra[i].w));
                uint2 q1, q2, q3;
                // branch-free zero padding (a divergent branch around the loaded registers makes hipcc
                // drain vmcnt(0) before the next prefetch: see the fp32 loader)
                const bool ok = (okm >> i) & 1u;
                if (PRO) {
                    // BN FMAs; ReLU and the padding select as ONE median per element:
                    // valid rows clamp to [0 or -inf, +inf), padded rows to [0, 0]
                    const sp_f32x2 a = {fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y)};
                    const sp_f32x2 b = {fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w)};
                    const float lo = ok ? lo_valid : 0.f, hi = ok ? __builtin_inff() : 0.f;
                    v.x = __builtin_amdgcn_fmed3f(a.x, lo, hi); v.y = __builtin_amdgcn_fmed3f(a.y, lo, hi);
                    v.z = __builtin_amdgcn_fmed3f(b.x, lo, hi); v.w = __builtin_amdgcn_fmed3f(b.y, lo, hi);
                } else {
                    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
                }
                __bf16* dst = A6 + ((size_t)(buf * NPL) * BM + lrow + 64 * i) * PITCH6 + kc * 4;
                if (F16) {
                    if (!PRO) { v.x *= sa; v.y *= sa; v.z *= sa; v.w *= sa; }
                    split4h(v, q1, q2);
                    *reinterpret_cast<uint2*>(dst) = q1;
                    *reinterpret_cast<uint2*>(dst + BM * PITCH6) = q2;
                } else {
                    split4(v, q1, q2, q3);
                    *reinterpret_cast<uint2*>(dst) = q1;
                    *reinterpret_cast<uint2*>(dst + BM * PITCH6) = q2;
                    *reinterpret_cast<uint2*>(dst + 2 * BM * PITCH6) = q3;
                }
            }
            if (brow < BN) {
#pragma unroll
                for (int j = 0; j < NPL; ++j)
                    *reinterpret_cast<u32x4*>(B6 + ((size_t)(buf * NPL + j) * BN + brow) * PITCH6 + bhalf * 8) = sb_.rb[j];
            }
        };
        // No conditionals around the loads and stores of the main loop: hipcc's vmcnt bookkeeping is exact only on
        // straight-line code (a guarded prefetch made it wait for vmcnt(0) before every LDS store).  Phase i = 1 .. nsteps
        // stores K-step i into buffer i & 1 (the MFMA waves are on step i - 1), then refills the A stage with step
        // i + DA and the B stage with step i + 2; the loop is unrolled over P = lcm(DA, 2) phases so that stage and
        // buffer indices are compile-time constants.
        constexpr int P = (DA % 2 == 0) ? DA : 2 * DA;
#pragma unroll
        for (int d = 0; d < DA; ++d) gloadA(SA[d]);
        gloadB(SB[0]);
        gloadB(SB[1]);
        if (PRO) {                                   // the BatchNorm vectors -> LDS, once
            for (int c = ltid; c < p.Cin; c += 256) {
                SS[c] = p.in_scale[c] * sa;
                SS[p.Cin + c] = p.in_shift[c] * sa;
            }
        }
        __syncthreads();                             // (all eight waves) SS is in place
        lstore(SA[0], SB[0], 0);
        gloadA(SA[0]);
        gloadB(SB[0]);
        __syncthreads();
        int i = 1;
        for (; i + P - 1 <= nsteps; i += P) {
#pragma unroll
            for (int u = 0; u < P; ++u) {
                lstore(SA[(1 + u) % DA], SB[(1 + u) & 1], (1 + u) & 1);
                gloadA(SA[(1 + u) % DA]);
                gloadB(SB[(1 + u) & 1]);
                __syncthreads();
            }
        }
        // up to P - 1 phases left (uniform branches; nothing is prefetched any more)
#pragma unroll
        for (int u = 0; u < P - 1; ++u)
            if (i + u <= nsteps) {
                lstore(SA[(1 + u) % DA], SB[(1 + u) & 1], (1 + u) & 1);
                __syncthreads();
            }
    } else {
        // ------------------------------------------------------------------ MFMA waves
        struct Frag { bf16x8 a[TM][3], b[TN][3]; };
        Frag F;
        auto rd = [&](Frag& f, int buf) {
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                for (int a = 0; a < TM; ++a)
                    f.a[a][pl] = *reinterpret_cast<const bf16x8*>(
                        A6 + ((size_t)(buf * NPL + pl) * BM + (wm * TM + a) * 32 + lr) * PITCH6 + 8 * lh);
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    f.b[b][pl] = *reinterpret_cast<const bf16x8*>(
                        B6 + ((size_t)(buf * NPL + pl) * BN + (wn * TN + b) * 32 + lr) * PITCH6 + 8 * lh);
            }
        };
        auto mm = [&](const Frag& f) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) mma_split<F16>(acc[a][b], f.a[a], f.b[b]);
        };
        __syncthreads();                   // the loaders' BatchNorm vectors are in LDS
        __syncthreads();                   // K-step 0 is staged
        for (int s = 0; s < nsteps; ++s) {
            rd(F, s & 1);
            mm(F);
            __syncthreads();
        }
    }
    conv_epilogue<WM, WN, TM, TN>(p, acc, smem, mtile, ntile, tid, wave, lane);
}

extern "C" int dsnt_conv_bf16x6_ok(const dsnt_conv_geom* g) {
    if (!g) return 0;
    return g->Cin % BK6 == 0 && g->Cout % 4 == 0 && g->R * g->S * 2 <= 32 &&
           (size_t)g->N * g->H * g->W * g->Cin * 4u < (1ull << 31) &&
           (size_t)3 * g->Cout * g->R * g->S * g->Cin * 2u < (1ull << 31);
}

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution on bf16x6 with an LDS halo tile.
//
// Why: VALU issue on a SIMD is arbitrated by priority, then age, and a wave issuing MFMAs back to back
// keeps winning: the loader waves' VALU work only runs in the gaps (tools/starve.py: a 128-instruction
// VALU burst next to a saturated matrix pipe takes the whole MFMA phase to finish).  In the implicit-GEMM
// kernel (conv_fwd_bf16x6_kernel) every filter tap re-loads, re-normalises and re-splits the same input pixels (9x the
// VALU work, 2.4x the HBM traffic of the tensor).  Here a workgroup owns an 8 x 16 patch of output
// pixels: the (8+2) x (16+2) input halo of 16 channels is transformed and split ONCE into LDS, then all
// nine taps run from it with shifted fragment addresses (immediate offsets), while only the pre-split
// weights stream through the double-buffered B tile (a 16-byte copy, no VALU).
// (A variant without the loader/MFMA role split — 256 threads, fragments of step s+1 read during the
// MFMAs of step s — reached 84 % matrix-pipe use inside the K loop but was 8 % slower end to end: with
// 72 K-steps per tile the ~10k-cycle prologue and ~12k-cycle epilogue of two lock-stepped workgroups
// per CU dominate either way.)
//   LDS: A halo [3 planes][192 px][24] bf16 (27.6 KB, single buffer: refilled at chunk boundaries
//   from registers that were loaded nine steps earlier) + B [2][3][BN][24] bf16 (36.9 KB).
// K order is (16-channel chunk, tap) instead of (tap, channel): same products, different fp32
// summation order than the implicit-GEMM kernel (differences at the 1e-7 level).
template <int TN, bool PRO, bool F16 = false>
__global__ __launch_bounds__(512, 2) void conv3x3_bf16x6_kernel(ConvP p) {
    constexpr int NPL = F16 ? 2 : 3;            // operand planes (fp16x3: two fp16 planes, three MFMAs)
    // fp16x3: the two-plane halo is small enough to be DOUBLE-buffered (2 x 18 KB + 24 KB of weights < the 66 KB the
    // epilogue's C tile needs anyway): the next chunk's halo is staged while this chunk's taps run, instead of in an
    // extra barrier-bracketed stage between chunks (which, with half the MFMAs per tap, had become 10 % of the kernel)
    constexpr int ABUF = F16 ? 2 : 1;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr int WN = 2, TM = 2, BM = 128, BN = WN * TN * 32;
    constexpr int HWD = 18, HPP = 192;                 // halo row width; halo pixels (180) padded to 192
    constexpr int BROWS = BN * 2 / 256 >= 1 ? 3 : 3;   // three planes per loader thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* A6 = reinterpret_cast<__bf16*>(smem);          // [ABUF][NPL][HPP][PITCH6]
    __bf16* B6 = A6 + ABUF * NPL * HPP * PITCH6;           // [2][NPL][BN][PITCH6]

    int tile;
    xcd_remap(blockIdx.x, p.mtiles * p.ntiles, tile);
    const int ntile = tile % p.ntiles, mtile = tile / p.ntiles;
    const int tws = p.W >> 4, ths = p.H >> 3;
    const int tw = mtile % tws, th = (mtile / tws) % ths, img = mtile / (tws * ths);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchunks = p.Cin >> 4;                    // even (Cin % 32 == 0)
    const int lr = lane & 31, lh = lane >> 5;
    const int cw = wave & 3;
    const int wm = cw >> 1, wn = cw & 1;
    (void)BROWS;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    if (wave >= 4) {
        // ------------------------------------------------------------------ loader waves
        const int ltid = tid - 256;
        const int kc = ltid & 3;
        const unsigned OOB = 0xF0000000u;
        unsigned aoffs[3], alds[3], aok = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int pix = (ltid >> 2) + 64 * i;      // 0..191, halo pixels 0..179
            const int hy = pix / HWD, hx = pix - hy * HWD;
            const int ih = th * 8 - 1 + hy, iw = tw * 16 - 1 + hx;
            const bool in = pix < 180 && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            aoffs[i] = in ? (unsigned)(((img * p.H + ih) * p.W + iw) * p.Cin + kc * 4) * 4u : OOB;
            alds[i] = (unsigned)(pix * PITCH6 + kc * 4);
            aok |= (in ? 1u : 0u) << i;
        }
        const int bhalf = ltid & 1;
        const int brow = ((ltid >> 4) << 3) + (((ltid >> 1) & 3) << 1) + ((ltid >> 3) & 1);
        const int bn = ntile * BN + brow;
        const bool bvalid = brow < BN && bn < p.Cout;
        unsigned bpix[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            bpix[j] = bvalid ? (unsigned)((size_t)j * p.wq_stride + (size_t)bn * p.K + bhalf * 8) * 2u : OOB;
        const unsigned blds = (unsigned)(brow * PITCH6 + bhalf * 8);
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.x), 0, (int)((size_t)p.N * p.H * p.W * p.Cin * 4u), 0x00020000);
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<unsigned short*>(p.wq), 0, (int)(((size_t)(NPL - 1) * p.wq_stride + (size_t)p.Cout * p.K) * 2u), 0x00020000);
        const float sa = F16 ? pow2_scale(bound64(p.a_bound)) : 1.f;      // fp16x3 operand scale
        u32x4 ra[3], rb[2][NPL];
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        const int lastc = nchunks - 1;
        const float lo_valid = p.in_relu ? 0.f : -__builtin_inff();
        auto gloadA = [&](int c) {
            c = min(c, lastc);
            if (PRO) {
                sc = *reinterpret_cast<const float4*>(p.in_scale + c * 16 + kc * 4);
                sh = *reinterpret_cast<const float4*>(p.in_shift + c * 16 + kc * 4);
                if (F16) {      // the operand scale rides in the BN vectors
                    sc.x *= sa; sc.y *= sa; sc.z *= sa; sc.w *= sa;
                    sh.x *= sa; sh.y *= sa; sh.z *= sa; sh.w *= sa;
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, aoffs[i], c * 64, 0);
        };
        auto storeA = [&](int abuf) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float4 v = make_float4(__uint_as_float(ra[i].x), __uint_as_float(ra[i].y),
                                       __uint_as_float(ra[i].z), __uint_as_float(ra[i].w));
                if (PRO) {
                    // BN FMAs; ReLU + zero padding (applied after BN + ReLU) as one median per element
                    const sp_f32x2 a = {fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y)};
                    const sp_f32x2 b = {fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w)};
                    const bool ok = (aok >> i) & 1u;
                    const float lo = ok ? lo_valid : 0.f, hi = ok ? __builtin_inff() : 0.f;
                    v.x = __builtin_amdgcn_fmed3f(a.x, lo, hi); v.y = __builtin_amdgcn_fmed3f(a.y, lo, hi);
                    v.z = __builtin_amdgcn_fmed3f(b.x, lo, hi); v.w = __builtin_amdgcn_fmed3f(b.y, lo, hi);
                }
                uint2 q1, q2, q3;
                __bf16* dst = A6 + abuf * NPL * HPP * PITCH6 + alds[i];
                if (F16) {
                    if (!PRO) { v.x *= sa; v.y *= sa; v.z *= sa; v.w *= sa; }
                    split4h(v, q1, q2);
                    *reinterpret_cast<uint2*>(dst) = q1;
                    *reinterpret_cast<uint2*>(dst + HPP * PITCH6) = q2;
                } else {
                    split4(v, q1, q2, q3);
                    *reinterpret_cast<uint2*>(dst) = q1;
                    *reinterpret_cast<uint2*>(dst + HPP * PITCH6) = q2;
                    *reinterpret_cast<uint2*>(dst + 2 * HPP * PITCH6) = q3;
                }
            }
        };
        // weights of K-step (chunk c, tap t): OHWI columns t*Cin + c*16 .. +16 of the three planes
        auto gloadB = [&](int stage, int c, int t) {
            c = min(c, lastc);
            const unsigned koff = (unsigned)(t * p.Cin + c * 16) * 2u;
#pragma unroll
            for (int j = 0; j < NPL; ++j) rb[stage][j] = __builtin_amdgcn_raw_buffer_load_b128(wr, bpix[j], koff, 0);
        };
        auto storeB = [&](int stage, int buf) {
            if (brow < BN) {
#pragma unroll
                for (int j = 0; j < NPL; ++j)
                    *reinterpret_cast<u32x4*>(B6 + (size_t)(buf * NPL + j) * BN * PITCH6 + blds) = rb[stage][j];
            }
        };
        // step s = 9 * chunk + tap reads B buffer s & 1; its weights sit in register stage s & 1
        gloadA(0);
        gloadB(0, 0, 0);
        gloadB(1, 0, 1);
        storeA(0);
        storeB(0, 0);
        gloadA(1);
        gloadB(0, 0, 2);
        __syncthreads();
        for (int c2 = 0; c2 < nchunks; c2 += 2) {
#pragma unroll
            for (int j = 0; j < 18; ++j) {
                // while the MFMA waves work on step j: stage step j+1, fetch step j+3
                storeB((j + 1) & 1, (j + 1) & 1);
                gloadB((j + 1) & 1, c2 + (j + 3) / 9, (j + 3) % 9);
                if (ABUF == 2) {
                    if (j % 9 == 0) {                // the other halo buffer is free since the last barrier
                        storeA(1 - (j / 9));
                        gloadA(c2 + j / 9 + 2);
                    }
                } else if (j % 9 == 8) {
                    __syncthreads();                 // the MFMA waves hold the last fragments of this chunk
                    storeA(0);
                    gloadA(c2 + j / 9 + 2);
                }
                __syncthreads();
            }
        }
    } else {
        // ------------------------------------------------------------------ MFMA waves
        struct Frag { bf16x8 a[TM][3], b[TN][3]; };
        Frag F;
        int aoff[TM], boff[TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
            // lanes 16..31 sit one halo row (18 pixels) further: rotating their pixel column by two restores
            // the 16-pixel period of the conflict-free ds_read_b128 pattern (26 % -> ~0 % bank conflicts)
            aoff[a] = (((wm * TM + a) * 2 + (lr >> 4)) * HWD + ((lr + (lr >> 4) * 14) & 15)) * PITCH6 + 8 * lh;
#pragma unroll
        for (int b = 0; b < TN; ++b) boff[b] = ((wn * TN + b) * 32 + lr) * PITCH6 + 8 * lh;
        __syncthreads();
        for (int c2 = 0; c2 < nchunks; c2 += 2) {
#pragma unroll
            for (int j = 0; j < 18; ++j) {
                const int t = j % 9, buf = j & 1;
                const int toff = ((t / 3) * HWD + (t % 3)) * PITCH6 + (ABUF == 2 ? (j / 9) * NPL * HPP * PITCH6 : 0);
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                    for (int a = 0; a < TM; ++a)
                        F.a[a][pl] = *reinterpret_cast<const bf16x8*>(A6 + pl * HPP * PITCH6 + aoff[a] + toff);
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        F.b[b][pl] = *reinterpret_cast<const bf16x8*>(B6 + (buf * NPL + pl) * BN * PITCH6 + boff[b]);
                }
                if (ABUF == 1 && t == 8) __syncthreads();   // fragments are in registers: the halo may be refilled
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b) mma_split<F16>(acc[a][b], F.a[a], F.b[b]);
                __syncthreads();
            }
        }
    }
    const int mbase = (img * p.H + th * 8) * p.W + tw * 16;
    conv_epilogue<2, WN, TM, TN, true>(p, acc, smem, mtile, ntile, tid, wave, lane, mbase);
}

template <int TN, bool F16 = false>
static void launch_conv3x3_6(const ConvP& p, bool pro, hipStream_t st) {
    constexpr int BN = 64 * TN, NPL = F16 ? 2 : 3;
    size_t lds = (size_t)((F16 ? 2 : 1) * NPL * 192 + 2 * NPL * BN) * PITCH6 * 2;
    const size_t epi = (size_t)128 * (BN + 4) * 4;
    if (epi > lds) lds = epi;
    if (lds > 65536) {
        DSNT_SET_MAX_LDS((conv3x3_bf16x6_kernel<TN, true, F16>), lds);
        DSNT_SET_MAX_LDS((conv3x3_bf16x6_kernel<TN, false, F16>), lds);
    }
    dim3 gr(p.mtiles * p.ntiles), bl(512);
    if (pro) DSNT_LAUNCH((conv3x3_bf16x6_kernel<TN, true, F16>), gr, bl, lds, st, p);
    else DSNT_LAUNCH((conv3x3_bf16x6_kernel<TN, false, F16>), gr, bl, lds, st, p);
}

static bool conv3x3_halo_ok(const dsnt_conv_geom* g) {
    return g->R == 3 && g->S == 3 && g->stride == 1 && g->pad == 1 && g->dil == 1 && g->Ho == g->H && g->Wo == g->W &&
           g->H % 8 == 0 && g->W % 16 == 0 && g->Cin % 32 == 0;
}

template <int WM, int WN, int TM, int TN, bool F16 = false>
static void launch_fwd6(const ConvP& p, bool pro, hipStream_t st) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    size_t lds = (size_t)2 * (F16 ? 2 : 3) * (BM + BN) * PITCH6 * 2 + (size_t)2 * p.Cin * sizeof(float);   // tiles + BN vectors
    const size_t epi = (size_t)BM * (BN + 4) * 4;          // the epilogue's C tile lives in the same LDS
    if (epi > lds) lds = epi;
    if (lds > 65536) {
        DSNT_SET_MAX_LDS((conv_fwd_bf16x6_kernel<WM, WN, TM, TN, true, F16, 2>), lds);
        DSNT_SET_MAX_LDS((conv_fwd_bf16x6_kernel<WM, WN, TM, TN, false, F16, 2>), lds);
    }
    // two A-operand register stages (DA): four measured 2-5 % slower on every 1x1 shape of the hourglass (round 2)
    dim3 gr(p.mtiles * p.ntiles), bl(512);
    if (pro) DSNT_LAUNCH((conv_fwd_bf16x6_kernel<WM, WN, TM, TN, true, F16, 2>), gr, bl, lds, st, p);
    else DSNT_LAUNCH((conv_fwd_bf16x6_kernel<WM, WN, TM, TN, false, F16, 2>), gr, bl, lds, st, p);
}

#ifndef FWD6_BN64_ROWS_DEFAULT
#define FWD6_BN64_ROWS_DEFAULT 8192
#endif

static int conv_fwd6_impl(const float* x, const void* w_planes, int64_t plane_stride, const float* bias, float* y,
                          const float* in_scale, const float* in_shift, int in_relu,
                          const float* res1, const float* res2, float* stats_partial,
                          const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* g_bnb, const dsnt_out_bounds* g_tail,
                          void* stream, const float* a_bound = nullptr, const float* w_bound = nullptr,
                          bool stream_w = false, const dsnt_bn_bwd_apply* g_ap = nullptr, float* ap_out = nullptr) {
    ConvP p;
    if (int e = conv_fill(p, "dsnt_conv_fwd_bf16x6", x, w_planes, true, plane_stride, bias, y, in_scale, in_shift, in_relu, res1, res2,
                          stats_partial, g, g_bnb, g_tail)) return e;
    // 64-column tiles also for wider outputs when there are few row tiles (the 16 x 16 level and below: 32-64 workgroups of 128 x 128
    // on 256 CUs, each a prologue + 8-16 K-steps + an epilogue through LDS): twice the workgroups, half the epilogue each.
    // DSNT_X_FWD6_BN64_ROWS: A/B
    static long bn64_rows = -1;
    if (bn64_rows < 0) { const char* e = getenv("DSNT_X_FWD6_BN64_ROWS"); bn64_rows = e ? atol(e) : FWD6_BN64_ROWS_DEFAULT; }
    const int BN = (g->Cout <= 64 || (p.M <= bn64_rows && g->Cout % 64 == 0 && !conv3x3_halo_ok(g))) ? 64 : 128;
    p.mtiles = (p.M + 127) / 128; p.ntiles = (p.Cout + BN - 1) / BN;
    hipStream_t st = (hipStream_t)stream;
    p.a_bound = a_bound; p.w_bound = w_bound;
    const bool share_chip = a_bound && (in_relu & DSNT_CONV_SHARE_CHIP) != 0;       // (fp16x3 entry points) leave room beside this launch
    if (a_bound) p.in_relu = in_relu & 1;
    if (g_ap) {
        p.ap_y = g_ap->y; p.ap_scale = g_ap->scale; p.ap_mean = g_ap->mean; p.ap_invstd = g_ap->invstd; p.ap_coef = g_ap->coef;
        p.ap_out = ap_out;
    }
    if (stream_w) {                  // 3x3, weights in the stream layout: the symmetric kernel (conv3s.hip)
        DSNT_REQUIRE(dsnt_conv3s_ok(p), DSNT_ERR_SHAPE, "dsnt_conv_fwd_f16x3_stream: launch not supported (dsnt_conv_fwd_stream_ok; "
                     "no second residual)");
        dsnt_conv3s_launch(p, in_scale != nullptr, st, share_chip);
        DSNT_CHECK_LAUNCH("dsnt_conv_fwd_f16x3_stream");
    }
    if (a_bound) {                   // fp16x3: two fp16 weight planes, operand bounds in device memory
        const int ntw = dsnt_gemm1_cfg(p);      // large 1x1 convolutions: the streaming kernel (gemm1.hip)
        if (ntw > 0) {
            dsnt_gemm1_launch(p, ntw, in_scale != nullptr, st, share_chip);
            DSNT_CHECK_LAUNCH("dsnt_conv_fwd_f16x3");
        }
        if (conv3x3_halo_ok(g)) {
            if (BN == 128) launch_conv3x3_6<2, true>(p, in_scale != nullptr, st);
            else launch_conv3x3_6<1, true>(p, in_scale != nullptr, st);
        } else if (BN == 128) launch_fwd6<2, 2, 2, 2, true>(p, in_scale != nullptr, st);
        else launch_fwd6<2, 2, 2, 1, true>(p, in_scale != nullptr, st);
    } else if (conv3x3_halo_ok(g)) {
        if (BN == 128) launch_conv3x3_6<2>(p, in_scale != nullptr, st);
        else launch_conv3x3_6<1>(p, in_scale != nullptr, st);
    } else if (BN == 128) launch_fwd6<2, 2, 2, 2>(p, in_scale != nullptr, st);
    else launch_fwd6<2, 2, 2, 1>(p, in_scale != nullptr, st);
    DSNT_CHECK_LAUNCH("dsnt_conv_fwd_bf16x6");
}

extern "C" int dsnt_conv_fwd_bf16x6(const float* x, const void* w_planes, int64_t plane_stride, const float* bias, float* y,
                                    const float* in_scale, const float* in_shift, int in_relu,
                                    const float* res1, const float* res2, float* stats_partial,
                                    const dsnt_conv_geom* g, void* stream) {
    return conv_fwd6_impl(x, w_planes, plane_stride, bias, y, in_scale, in_shift, in_relu, res1, res2,
                          stats_partial, g, nullptr, nullptr, stream);
}

extern "C" int dsnt_conv_fwd_bf16x6_ex(const float* x, const void* w_planes, int64_t plane_stride, const float* bias,
                                       float* y, const float* in_scale, const float* in_shift, int in_relu,
                                       const float* res1, const float* res2, float* stats_partial,
                                       const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail,
                                       void* stream) {
    return conv_fwd6_impl(x, w_planes, plane_stride, bias, y, in_scale, in_shift, in_relu, res1, res2,
                          stats_partial, g, bnb, tail, stream);
}

extern "C" int dsnt_conv_fwd_f16x3_ex(const float* x, const void* w_planes, int64_t plane_stride, const float* w_bound,
                                      const float* a_bound, const float* bias, float* y, const float* in_scale,
                                      const float* in_shift, int in_relu, const float* res1, const float* res2,
                                      float* stats_partial, const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb,
                                      const dsnt_out_bounds* tail, void* stream) {
    DSNT_REQUIRE(a_bound && w_bound, DSNT_ERR_ARG, "dsnt_conv_fwd_f16x3_ex: the operand bounds (device scalars) are required");
    return conv_fwd6_impl(x, w_planes, plane_stride, bias, y, in_scale, in_shift, in_relu, res1, res2,
                          stats_partial, g, bnb, tail, stream, a_bound, w_bound);
}

// The same call with the weight planes in the STREAM layout of dsnt_f16_prep_weights (3x3 convolutions the symmetric
// kernel of conv3s.hip runs: dsnt_conv_fwd_stream_ok)
extern "C" int dsnt_conv_fwd_f16x3_stream(const float* x, const void* w_planes, int64_t plane_stride, const float* w_bound,
                                          const float* a_bound, const float* bias, float* y, const float* in_scale,
                                          const float* in_shift, int in_relu, const float* res1, const float* res2,
                                          float* stats_partial, const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb,
                                          const dsnt_out_bounds* tail, void* stream) {
    DSNT_REQUIRE(a_bound && w_bound, DSNT_ERR_ARG, "dsnt_conv_fwd_f16x3_stream: the operand bounds (device scalars) are required");
    return conv_fwd6_impl(x, w_planes, plane_stride, bias, y, in_scale, in_shift, in_relu, res1, res2,
                          stats_partial, g, bnb, tail, stream, a_bound, w_bound, true);
}
extern "C" int dsnt_conv_fwd_stream_ok(const dsnt_conv_geom* g) { return dsnt_conv3s_geom_ok(g) ? 1 : 0; }
extern "C" int dsnt_conv_fwd_stream_form(const dsnt_conv_geom* g, int mode) { return dsnt_conv3s_form_of(g, mode); }

// The data gradient of a 3x3 convolution whose OUTPUT feeds a train-mode BatchNorm, with that BatchNorm's backward folded into
// the operand load (conv3s.hip MODE 4): instead of dL/dy the launch reads dz (the ReLU-masked, reduced gradient behind the
// BatchNorm) and the BatchNorm's input ap->y and forms  dy = scale (dz - c0 - (y - mean) invstd c1)  on the fly; it also writes
// dy to dy_out (what the weight gradient of the same convolution reads next).  bnb (required): the BatchNorm-backward epilogue
// of the BatchNorm IN FRONT of the convolution, as in dsnt_conv_fwd_f16x3_stream.  a_bound: a bound of |dy|
// (dsnt_bn_bwd_finalize_bound).
extern "C" int dsnt_conv_dgrad_f16x3_stream_apply(const float* dz, const dsnt_bn_bwd_apply* ap, float* dy_out,
                                                  const void* w_planes, int64_t plane_stride, const float* w_bound,
                                                  const float* a_bound, float* dx_dz, float* stats_partial, int flags,
                                                  const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb,
                                                  const dsnt_out_bounds* tail, void* stream) {
    DSNT_REQUIRE(a_bound && w_bound, DSNT_ERR_ARG, "dsnt_conv_dgrad_f16x3_stream_apply: the operand bounds (device scalars) are required");
    DSNT_REQUIRE(ap && ap->y && ap->scale && ap->mean && ap->invstd && ap->coef && dy_out && bnb, DSNT_ERR_ARG,
                 "dsnt_conv_dgrad_f16x3_stream_apply: needs a complete dsnt_bn_bwd_apply, dy_out and the BatchNorm-backward epilogue");
    DSNT_REQUIRE(dsnt_aligned16(ap->y) && dsnt_aligned16(dy_out) && dy_out != dz, DSNT_ERR_ALIGN,
                 "dsnt_conv_dgrad_f16x3_stream_apply: 16-byte alignment; dy_out must not alias dz (halo pixels are re-read by other workgroups)");
    return conv_fwd6_impl(dz, w_planes, plane_stride, nullptr, dx_dz, nullptr, nullptr, flags & DSNT_CONV_SHARE_CHIP, nullptr, nullptr,
                          stats_partial, g, bnb, tail, stream, a_bound, w_bound, true, ap, dy_out);
}

// Which kernel an fp16x3 launch of this geometry reaches (both operand bounds given, no second residual, no BatchNorm-backward
// epilogue).  wgrad = 0, dsnt_conv_fwd_f16x3_ex: 1 the streaming 1x1 kernel (gemm1.hip), 2 the LDS halo-tile kernel, 0 the implicit
// GEMM.  wgrad = 1, dsnt_conv_wgrad_f16x3: 1 the stem kernel (stem4.hip), 2 the halo kernel (wgrad3.hip), 3 the 1x1 kernel
// (wgrad1.hip), 0 the generic one.  Negative: the geometry is not supported.
extern "C" int dsnt_conv_f16x3_route(const dsnt_conv_geom* g, int wgrad) {
    if (!g || conv_check_geom(g, "dsnt_conv_f16x3_route") != 0) return -1;
    if (wgrad) return dsnt_wgrad_route_kind(g);       // the route of conv_wgrad.hip itself
    if (!dsnt_conv_bf16x6_ok(g)) return -1;
    static const float one = 1.f;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.a_bound = &one; p.w_bound = &one; p.wq = reinterpret_cast<const unsigned short*>(&one);
    conv_geom_fill(p, g);
    if (dsnt_gemm1_cfg(p) > 0) return 1;
    return conv3x3_halo_ok(g) ? 2 : 0;
}
