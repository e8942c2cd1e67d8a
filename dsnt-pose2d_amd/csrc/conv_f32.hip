// Implicit-GEMM convolutions on the fp32 matrix cores of gfx950
// (v_mfma_f32_32x32x2_f32: exact f32, bit-for-bit a k-ordered fmaf chain).
//
// Forward / data-gradient:   Y[M][Cout] = act(im2col(X))[M][K] * W^T[K][Cout] (+bias +res1 +res2)
//   M = N*Ho*Wo, K = R*S*Cin, X is NHWC, W is OHWI (= [Cout][K], K contiguous).
//   The BatchNorm+ReLU that precedes the conv (pre-activation Bottleneck) is applied while the
//   A tile is staged (scale/shift per input channel), zero padding after the activation.
//   Epilogue: bias, up to two residual adds, and per-tile column sums / sums of squares of Y
//   (the next BatchNorm's batch statistics), so no separate pass over Y is needed.
// (The split-precision forms of the same contract: conv_split6.hip; the weight gradients: conv_wgrad.hip.)
// Also here: the K-split kernel for few output rows.
//
// Tiling: 256 threads = 4 waves (one per SIMD); every wave owns TM x TN tiles of 32x32
// accumulators; BK = 32.  LDS tiles are k-contiguous with a 36-float pitch so that the
// ds_read_b128 fragment reads (lane (r,h) reads 4 consecutive k at row r, k-offset 4h) are
// bank-conflict free.  One barrier per K-step, global loads for step s+1 in flight during the
// MFMAs of step s (register staging: the A operand needs per-element BN/ReLU/padding).
#include "conv_epilogue.h"
#include <string.h>
#include <stdlib.h>

#define BK 32
#define PITCH 36

// Wave-specialised: a workgroup is 8 waves — waves 0..3 only read fragments from LDS and issue
// MFMAs (one per SIMD, 64 MFMAs = 4096 matrix-pipe cycles per K-step), waves 4..7 only move data
// (global loads two K-steps ahead, BN+ReLU / zero-padding transform, LDS stores).  The two roles
// meet at one barrier per K-step, so the matrix pipe never waits on address arithmetic, memory
// latency or the transform.  Two workgroups per CU (LDS-limited) give each SIMD two MFMA waves.
// FAST (Cin % 32 == 0, R*S*APASS <= 64, tensors < 4 GiB): the filter tap of a K-step is
// wave-uniform, so loader addresses are a per-thread constant plus a scalar — range-checked buffer
// loads need one v_add per 16-byte load and no clamping, and zero padding comes from a validity
// bit-mask computed once per thread.  This matters because on gfx950 the fp32 MFMA executes at the
// vector-FP32 rate and loader VALU instructions measurably take matrix-pipe time.
template <int WM, int WN, int TM, int TN, bool PRO, bool FAST>
__global__ __launch_bounds__(512, 4) void conv_fwd_kernel(ConvP p) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int APASS = BM / 32, BPASS = BN / 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][BM][PITCH]
    float* Bs = smem + 2 * BM * PITCH;      // [2][BN][PITCH]

    int tile;
    xcd_remap(blockIdx.x, p.mtiles * p.ntiles, tile);
    const int ntile = tile % p.ntiles, mtile = tile / p.ntiles;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nsteps = (p.K + BK - 1) / BK;
    const int lr = lane & 31, lh = lane >> 5;
    const int cw = wave & 3;
    const int wm = cw / WN, wn = cw % WN;
    if (PRO && p.pro.partial) {          // the A operand's BatchNorm is finalised here (bn_pro.h: bn_pro_forward)
        bn_pro_forward<512>(p.pro, reinterpret_cast<double*>(smem), blockIdx.x == 0);
        __syncthreads();                 // this workgroup's stores to in_scale / in_shift are visible to its loads
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    if (FAST && wave >= 4) {
        // ------------------------------------------------------------------ loader waves (fast)
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const int ltid = tid - 256;
        const int lrow = ltid >> 3, kc = ltid & 7;
        const int HoWo = p.Ho * p.Wo;
        const int RS = p.R * p.S;
        // per-thread constants: byte offset of (row i, tap (0,0), channel 4*kc) and tap validity
        unsigned apix[APASS];
        unsigned long long vmask = 0ull;            // bit tap*APASS + i
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            const int m = mtile * BM + lrow + 32 * i;
            const bool vm = m < p.M;
            const int mm = vm ? m : 0;
            const int n = mm / HoWo, rem = mm - n * HoWo;
            const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
            const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
            apix[i] = (unsigned)(((n * p.H + ih0) * p.W + iw0) * p.Cin + kc * 4) * 4u;
            for (int t = 0; t < RS; ++t) {
                const int r = t / p.S, s_ = t - r * p.S;
                const int ih = ih0 + r * p.dil, iw = iw0 + s_ * p.dil;
                if (vm && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
                    vmask |= 1ull << (t * APASS + i);
            }
        }
        unsigned bpix[BPASS];
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            const int n = ntile * BN + lrow + 32 * j;
            bpix[j] = n < p.Cout ? (unsigned)(n * p.K + kc * 4) * 4u : 0xF0000000u;   // OOB -> 0
        }
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.x), 0, (int)((size_t)p.N * p.H * p.W * p.Cin * 4u), 0x00020000);
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.w), 0, (int)((size_t)p.Cout * p.K * 4u), 0x00020000);
        struct Stage {
            u32x4 ra[APASS], rb[BPASS];
            float4 sc, sh;
            unsigned ok;       // APASS validity bits of this step's tap
        };
        Stage S0, S1;
        auto gload = [&](Stage& st, int step) {
            // all scalar: tap, channel base, byte offset of the tap relative to tap (0,0)
            const int kb = step * BK;
            const int tap = kb / p.Cin, cb = kb - tap * p.Cin;
            const int r = tap / p.S, s_ = tap - r * p.S;
            const unsigned toff = (unsigned)(((r * p.dil) * p.W + s_ * p.dil) * p.Cin + cb) * 4u;
            if (PRO) {
                st.sc = *reinterpret_cast<const float4*>(p.in_scale + cb + kc * 4);
                st.sh = *reinterpret_cast<const float4*>(p.in_shift + cb + kc * 4);
            }
            st.ok = (unsigned)(vmask >> (tap * APASS));
#pragma unroll
            for (int i = 0; i < APASS; ++i)
                st.ra[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, apix[i] + toff, 0, 0);
            const unsigned koff = (unsigned)kb * 4u;
#pragma unroll
            for (int j = 0; j < BPASS; ++j)
                st.rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, bpix[j] + koff, 0, 0);
        };
        auto lstore = [&](const Stage& st, int buf) {
#pragma unroll
            for (int i = 0; i < APASS; ++i) {
                float4 v = make_float4(__uint_as_float(st.ra[i].x), __uint_as_float(st.ra[i].y),
                                       __uint_as_float(st.ra[i].z), __uint_as_float(st.ra[i].w));
                float* dst = As + (buf * BM + lrow + 32 * i) * PITCH + kc * 4;
                // branch-free on purpose: consuming the loaded registers inside a divergent branch makes
                // hipcc lose track of which loads have completed and drain vmcnt(0) before the next
                // prefetch is issued (seen in the ISA) — the register prefetch pipeline collapses
                if (PRO) {
                    v.x = fmaf(v.x, st.sc.x, st.sh.x); v.y = fmaf(v.y, st.sc.y, st.sh.y);
                    v.z = fmaf(v.z, st.sc.z, st.sh.z); v.w = fmaf(v.w, st.sc.w, st.sh.w);
                    if (p.in_relu) {
                        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
                        v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    }
                }
                const bool ok = (st.ok >> i) & 1u;
                v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
                *reinterpret_cast<float4*>(dst) = v;
            }
#pragma unroll
            for (int j = 0; j < BPASS; ++j)
                *reinterpret_cast<u32x4*>(Bs + (buf * BN + lrow + 32 * j) * PITCH + kc * 4) = st.rb[j];
        };
        // no conditionals around gload/lstore (see the bf16x6 loader): the tail re-loads the last step
        const int last = nsteps - 1;
        gload(S0, 0);
        gload(S1, min(1, last));
        lstore(S0, 0);
        gload(S0, min(2, last));
        __syncthreads();
        int s = 0;
        for (; s + 1 < nsteps; s += 2) {
            lstore(S1, 1);
            gload(S1, min(s + 3, last));
            __syncthreads();
            lstore(S0, 0);                 // s + 2 == nsteps: refills the idle buffer 0, harmless
            gload(S0, min(s + 4, last));
            __syncthreads();
        }
        if (s < nsteps) __syncthreads();
    } else if (wave >= 4) {
        // ------------------------------------------------------------------ loader waves (general)
        const int ltid = tid - 256;
        const int lrow = ltid >> 3, kc = ltid & 7;
        int abase[APASS], aih0[APASS], aiw0[APASS];
        const int HoWo = p.Ho * p.Wo;
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            const int m = mtile * BM + lrow + 32 * i;
            if (m < p.M) {
                const int n = m / HoWo, rem = m - n * HoWo;
                const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
                abase[i] = n * p.H * p.W * p.Cin;
                aih0[i] = oh * p.stride - p.pad;
                aiw0[i] = ow * p.stride - p.pad;
            } else {
                abase[i] = 0; aih0[i] = -(1 << 28); aiw0[i] = 0;
            }
        }
        int boff[BPASS];
        bool bok[BPASS];
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            const int n = ntile * BN + lrow + 32 * j;
            bok[j] = n < p.Cout;
            boff[j] = bok[j] ? n * p.K : 0;
        }
        // Two register sets: the loads of K-step s+2 and s+3 are in flight while s+1 is stored,
        // i.e. every global load has two full K-steps (>= 8k matrix-pipe cycles) to land.
        struct Stage {
            float4 ra[APASS], rb[BPASS];
            float4 sc, sh;
            unsigned okmask;
        };
        Stage S0, S1;
        // issue-only: unconditional loads from clamped addresses, nothing consumed here
        auto gload = [&](Stage& st, int step) {
            const int k0 = step * BK + kc * 4;
            const bool vk = k0 < p.K;
            const int tap = k0 / p.Cin, c = k0 - tap * p.Cin;
            const int r = tap / p.S, s = tap - r * p.S;
            const int dh = r * p.dil, dw = s * p.dil;
            if (PRO) {
                const int cc = vk ? c : 0;
                st.sc = *reinterpret_cast<const float4*>(p.in_scale + cc);
                st.sh = *reinterpret_cast<const float4*>(p.in_shift + cc);
            }
            st.okmask = 0;
#pragma unroll
            for (int i = 0; i < APASS; ++i) {
                const int ih = aih0[i] + dh, iw = aiw0[i] + dw;
                const bool ok = vk && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
                const int off = ok ? abase[i] + (ih * p.W + iw) * p.Cin + c : 0;
                st.ra[i] = *reinterpret_cast<const float4*>(p.x + off);
                st.okmask |= (ok ? 1u : 0u) << i;
            }
#pragma unroll
            for (int j = 0; j < BPASS; ++j) {
                const bool ok = vk && bok[j];
                st.rb[j] = *reinterpret_cast<const float4*>(p.w + (ok ? boff[j] + k0 : 0));
                st.okmask |= (ok ? 1u : 0u) << (8 + j);
            }
        };
        auto lstore = [&](const Stage& st, int buf) {
#pragma unroll
            for (int i = 0; i < APASS; ++i) {
                float4 v = st.ra[i];
                if (PRO) {
                    v.x = fmaf(v.x, st.sc.x, st.sh.x); v.y = fmaf(v.y, st.sc.y, st.sh.y);
                    v.z = fmaf(v.z, st.sc.z, st.sh.z); v.w = fmaf(v.w, st.sc.w, st.sh.w);
                    if (p.in_relu) {
                        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
                        v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    }
                }
                if (!((st.okmask >> i) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(As + (buf * BM + lrow + 32 * i) * PITCH + kc * 4) = v;
            }
#pragma unroll
            for (int j = 0; j < BPASS; ++j) {
                float4 v = st.rb[j];
                if (!((st.okmask >> (8 + j)) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(Bs + (buf * BN + lrow + 32 * j) * PITCH + kc * 4) = v;
            }
        };
        // no conditionals around gload/lstore (see the bf16x6 loader): the tail re-loads the last step
        const int last = nsteps - 1;
        gload(S0, 0);
        gload(S1, min(1, last));
        lstore(S0, 0);
        gload(S0, min(2, last));
        __syncthreads();
        // iteration s stores K-step s+1 (held in S1 for even s, S0 for odd s) into the buffer the
        // MFMA waves left in iteration s-1, then refills that register set with K-step s+3
        int s = 0;
        for (; s + 1 < nsteps; s += 2) {
            lstore(S1, 1);
            gload(S1, min(s + 3, last));
            __syncthreads();
            lstore(S0, 0);                 // s + 2 == nsteps: refills the idle buffer 0, harmless
            gload(S0, min(s + 4, last));
            __syncthreads();
        }
        if (s < nsteps) __syncthreads();     // odd step count: the last iteration only synchronises
    } else {
        // ------------------------------------------------------------------ MFMA waves
        __builtin_amdgcn_s_setprio(1);
        // Software-pipelined fragment reads: the ds_reads of k-group g+1 are issued before the 16
        // MFMAs of group g (two fragment register sets), and the barrier of a K-step sits in front
        // of its LAST group, so the first reads of the next step are already in flight while that
        // group's MFMAs run.  The matrix pipe then only idles for the barrier skew.
        struct Frag { float4 a[TM], b[TN]; };
        Frag F0, F1;
        auto rd = [&](Frag& f, int buf, int ks) {
            const float* Ab = As + (buf * BM + (wm * TM) * 32 + lr) * PITCH + 4 * lh + ks * 8;
            const float* Bb = Bs + (buf * BN + (wn * TN) * 32 + lr) * PITCH + 4 * lh + ks * 8;
#pragma unroll
            for (int a = 0; a < TM; ++a) f.a[a] = *reinterpret_cast<const float4*>(Ab + a * 32 * PITCH);
#pragma unroll
            for (int b = 0; b < TN; ++b) f.b[b] = *reinterpret_cast<const float4*>(Bb + b * 32 * PITCH);
        };
        auto mm = [&](const Frag& f) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[a].x, f.b[b].x, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[a].y, f.b[b].y, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[a].z, f.b[b].z, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[a].w, f.b[b].w, acc[a][b], 0, 0, 0);
                }
        };
        __syncthreads();
        rd(F0, 0, 0);
        for (int s = 0; s < nsteps; ++s) {
            const int buf = s & 1;
            rd(F1, buf, 1);
            __builtin_amdgcn_sched_barrier(0);
            mm(F0);
            __builtin_amdgcn_sched_barrier(0);
            rd(F0, buf, 2);
            __builtin_amdgcn_sched_barrier(0);
            mm(F1);
            __builtin_amdgcn_sched_barrier(0);
            rd(F1, buf, 3);
            __builtin_amdgcn_sched_barrier(0);
            mm(F0);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                       // all of this step's LDS reads have landed
            if (s + 1 < nsteps) rd(F0, buf ^ 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            mm(F1);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
    }

    conv_epilogue<WM, WN, TM, TN>(p, acc, smem, mtile, ntile, tid, wave, lane);
}

// ------------------------------------------------------------------------------------------
// tile configuration choice (shared with the Python side through dsnt_conv_fwd_bm)
static void pick_cfg(const dsnt_conv_geom* g, int& BM, int& BN) {
    const long M = (long)g->N * g->Ho * g->Wo;
    if (g->Cout <= 32) { BM = 128; BN = 32; }
    else if (g->Cout <= 64) { BM = 128; BN = 64; }
    else { BM = 128; BN = 128; }
    // few rows: trade register blocking for more workgroups
    const long tiles = ((M + BM - 1) / BM) * ((g->Cout + BN - 1) / BN);
    if (tiles < 256 && g->Cout >= 128) { BM = 32; BN = 128; }
}

extern "C" int dsnt_conv_fwd_bm(const dsnt_conv_geom* g) {
    int BM, BN;
    pick_cfg(g, BM, BN);
    return BM;
}

template <int WM, int WN, int TM, int TN>
static int launch_fwd(const ConvP& p, bool pro, hipStream_t st) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const size_t lds = (size_t)2 * (BM + BN) * PITCH * sizeof(float);
    const int grid = p.mtiles * p.ntiles;
    // one-time opt-in to > 64 KiB of dynamic LDS (not a stream operation; safe under capture)
    if (lds > 65536) {
        DSNT_SET_MAX_LDS((conv_fwd_kernel<WM, WN, TM, TN, true, true>), lds);
        DSNT_SET_MAX_LDS((conv_fwd_kernel<WM, WN, TM, TN, false, true>), lds);
        DSNT_SET_MAX_LDS((conv_fwd_kernel<WM, WN, TM, TN, true, false>), lds);
        DSNT_SET_MAX_LDS((conv_fwd_kernel<WM, WN, TM, TN, false, false>), lds);
    }
    const bool fast = (p.Cin % BK == 0) && (p.R * p.S * (BM / 32) <= 64) &&
                      ((size_t)p.N * p.H * p.W * p.Cin * 4u < (1ull << 31)) &&
                      ((size_t)p.Cout * p.K * 4u < (1ull << 31));
    dim3 gr(grid), bl(512);
    if (pro && fast) DSNT_LAUNCH((conv_fwd_kernel<WM, WN, TM, TN, true, true>), gr, bl, lds, st, p);
    else if (pro) DSNT_LAUNCH((conv_fwd_kernel<WM, WN, TM, TN, true, false>), gr, bl, lds, st, p);
    else if (fast) DSNT_LAUNCH((conv_fwd_kernel<WM, WN, TM, TN, false, true>), gr, bl, lds, st, p);
    else DSNT_LAUNCH((conv_fwd_kernel<WM, WN, TM, TN, false, false>), gr, bl, lds, st, p);
    return 0;
}

int conv_check_geom(const dsnt_conv_geom* g, const char* who) {
    DSNT_REQUIRE(g != nullptr, DSNT_ERR_ARG, "%s: null geometry", who);
    DSNT_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->Cin > 0 && g->Cout > 0 && g->R > 0 &&
                 g->S > 0 && g->stride > 0 && g->dil > 0 && g->pad >= 0, DSNT_ERR_SHAPE,
                 "%s: non-positive dimension", who);
    DSNT_REQUIRE(g->Cin % 4 == 0, DSNT_ERR_ALIGN, "%s: Cin=%d must be a multiple of 4", who, g->Cin);
    DSNT_REQUIRE(g->Cout % 4 == 0, DSNT_ERR_ALIGN, "%s: Cout=%d must be a multiple of 4", who, g->Cout);
    const int ho = (g->H + 2 * g->pad - g->dil * (g->R - 1) - 1) / g->stride + 1;
    const int wo = (g->W + 2 * g->pad - g->dil * (g->S - 1) - 1) / g->stride + 1;
    DSNT_REQUIRE(ho == g->Ho && wo == g->Wo, DSNT_ERR_SHAPE,
                 "%s: output %dx%d inconsistent with input/filter (expected %dx%d)", who, g->Ho,
                 g->Wo, ho, wo);
    DSNT_REQUIRE((long)g->N * g->H * g->W * g->Cin < (1L << 31) &&
                 (long)g->N * g->Ho * g->Wo * g->Cout < (1L << 31), DSNT_ERR_SHAPE,
                 "%s: tensor exceeds 2^31 elements", who);
    return DSNT_OK;
}

// ------------------------------------------------------------------------------------------
// Few output rows (the 8x8 and 4x4 hourglass levels: M = 2048 / 512 at batch 32): the tiled kernels above
// put one 32 x 32 accumulator per wave behind the WHOLE reduction (3x3 128->128: 576 dependent
// v_mfma_f32_32x32x2_f32 = 37 k cycles = ~18 us whatever the tile shape) on 16 ... 64 workgroups, i.e. most
// SIMDs idle.  Here a 512-thread workgroup owns ONE 32 x 32 output tile and its eight waves split K:
// every wave streams its K slice straight from global memory into MFMA operand registers (lane (i, h) holds
// row i, k = 8 j + 4 h .. + 3 of the A rows and of the weight rows: one 16-byte load each per four MFMAs, no
// LDS staging, no barrier in the loop), the eight partial tiles are summed through LDS in wave order
// (deterministic) and the usual epilogue (bias, residuals, statistics, BN-backward masking) runs on the sum.
// Same contract and statistics layout (32-row tiles) as conv_fwd_kernel<1, 4, 1, 1>.
// CW = k values per chunk and row (8, 16 or 32).  A lane (i, h) owns row i and CW / 2 consecutive k values of a chunk:
// CW / 8 16-byte loads per operand, issued back to back.  With CW = 8 the two lanes of a row use 32 bytes of a
// 128-byte line per load instruction, the next 32 bytes a whole MFMA batch (and 15 other waves' loads) later: the L1
// (32 KB against 16 waves x 64 lines in flight) has dropped the line by then, every chunk re-fetches it from L2, and the
// loads cost L1 fills at 4x the operand bytes on top of 32 tag look-ups per instruction (a lane is a row: the MFMA operand
// layout), which together take about as long as the MFMAs (3x3 256->256 at M = 2048: 49 us for 18 us of matrix pipe;
// deeper prefetch makes it worse: 57 / 70 us with 4 / 6 chunks in flight).  Measured, CW = 8 / 16 / 32: that launch 49 /
// 45 / 49 us, 3x3 512->512 at M = 512 51 / 43 / 41 us, the hourglass's 128-channel forms 18 / 16.5 / 18.8 us (CW = 32
// holds 96 load registers: occupancy 3-4 waves per SIMD); resnet34 batch 8 5.18 / 5.02 / 5.05 ms per step, hg2 batch 32
// 13.58 / 13.57 / 13.74 ms.  CW = 16 ships.  Needs Cin % CW == 0 (a chunk never straddles a filter tap); else CW = 8.
// (`part`: the kernel's 8 x 32 x 33 floats of LDS.  Still a device function under its kernel: with `part` named directly the two
// kernels with a BatchNorm prologue compile to 19 / 11 more instructions.)
template <bool PRO, int CW>
__device__ __forceinline__ void conv_ksplit_body(const ConvP& p, float (*part)[32][33]) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr int NL = CW / 8;                      // 16-byte loads per operand, lane and chunk
    const int nt32 = (p.Cout + 31) >> 5;
    const int tile = blockIdx.x;
    const int ntile = tile % nt32, mtile = tile / nt32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const unsigned OOB = 0xF0000000u;
    if (PRO && p.pro.partial) {          // the A operand's BatchNorm is finalised here (bn_pro.h: bn_pro_forward)
        bn_pro_forward<512>(p.pro, reinterpret_cast<double*>(&part[0][0][0]), tile == 0);
        __syncthreads();                 // this workgroup's stores to in_scale / in_shift are visible to its loads
    }
    // the BatchNorm vectors of the A operand live in LDS during the loop (in `part`, which is only written after it; Cin <=
    // 4096): as global loads inside the loop they would queue behind the prefetched chunks (loads return in order)
    float* const ssc = &part[0][0][0];
    if (PRO) {
        for (int c = tid; c < p.Cin; c += 512) { ssc[c] = p.in_scale[c]; ssc[p.Cin + c] = p.in_shift[c]; }
        __syncthreads();
    }
    // A row of this lane
    const int m = mtile * 32 + i;
    const bool vm = m < p.M;
    const int HoWo = p.Ho * p.Wo;
    const int mm = vm ? m : 0;
    const int img = mm / HoWo, rem = mm - img * HoWo;
    const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
    const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
    // weight row of this lane
    const int nb = ntile * 32 + i;
    const int kl = (CW / 2) * h;                    // this lane's k offset inside a chunk
    const unsigned boff = nb < p.Cout ? (unsigned)((size_t)nb * p.K + kl) * 4u : OOB;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x), 0, (int)((size_t)p.N * p.H * p.W * p.Cin * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.w), 0, (int)((size_t)p.Cout * p.K * 4u), 0x00020000);
    const int nch = p.K / CW;                       // a chunk never straddles a filter tap
    const int c0 = wave * nch / 8, c1 = (wave + 1) * nch / 8;
    const float lo_valid = p.in_relu ? 0.f : -__builtin_inff();
    struct Frag { u32x4 a[NL], b[NL]; bool ok; int cb; };
    // position of the next chunk to load (scalars; stepped, not divided: the loop's issue slots belong to the MFMAs —
    // fp32 MFMAs and VALU instructions exclude each other on a SIMD, profiles/r03_pmc_ksplit.txt); it stops at the
    // wave's last chunk, which the tail of the loop re-loads (never used) to stay straight-line
    int pos = c0, pr, ps, pcb;
    {
        const int kb = c0 * CW, tap = kb / p.Cin;
        pcb = kb - tap * p.Cin; pr = tap / p.S; ps = tap - pr * p.S;
    }
    auto load_next = [&]() {
        Frag f;
        const int ih = ih0 + pr * p.dil, iw = iw0 + ps * p.dil;
        f.ok = vm && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        f.cb = pcb;
        const unsigned aoff = f.ok ? (unsigned)(((img * p.H + ih) * p.W + iw) * p.Cin + pcb + kl) * 4u : OOB;
        const int kb4 = ((pr * p.S + ps) * p.Cin + pcb) * 4;
#pragma unroll
        for (int q = 0; q < NL; ++q) f.a[q] = __builtin_amdgcn_raw_buffer_load_b128(xr, aoff + 16u * q, 0, 0);
#pragma unroll
        for (int q = 0; q < NL; ++q) f.b[q] = __builtin_amdgcn_raw_buffer_load_b128(wr, boff + 16u * q, kb4, 0);
        if (pos < c1 - 1) {
            ++pos;
            pcb += CW;
            if (pcb == p.Cin) { pcb = 0; if (++ps == p.S) { ps = 0; ++pr; } }
        }
        return f;
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    auto mma = [&](const Frag& f) {
        const float lo = f.ok ? lo_valid : 0.f, hi = f.ok ? __builtin_inff() : 0.f;
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            float4 a = make_float4(__uint_as_float(f.a[q].x), __uint_as_float(f.a[q].y), __uint_as_float(f.a[q].z),
                                   __uint_as_float(f.a[q].w));
            if (PRO) {
                const float4 sc = *reinterpret_cast<const float4*>(ssc + f.cb + kl + 4 * q);
                const float4 sh = *reinterpret_cast<const float4*>(ssc + p.Cin + f.cb + kl + 4 * q);
                a.x = __builtin_amdgcn_fmed3f(fmaf(a.x, sc.x, sh.x), lo, hi);
                a.y = __builtin_amdgcn_fmed3f(fmaf(a.y, sc.y, sh.y), lo, hi);
                a.z = __builtin_amdgcn_fmed3f(fmaf(a.z, sc.z, sh.z), lo, hi);
                a.w = __builtin_amdgcn_fmed3f(fmaf(a.w, sc.w, sh.w), lo, hi);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, __uint_as_float(f.b[q].x), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, __uint_as_float(f.b[q].y), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, __uint_as_float(f.b[q].z), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, __uint_as_float(f.b[q].w), acc, 0, 0, 0);
        }
    };
    // the epilogue's operands (two rows per thread: rg, rg + 16 of column `col`) are fetched NOW, under the K loop: behind the
    // reduction every one of them is a dependent load on a launch whose whole length is the dependency chain's (round 5, box N)
    const int col = tid & 31, rg = tid >> 5;
    const int n = ntile * 32 + col;
    const bool vn = n < p.Cout;
    const bool bnb = p.bnb_scale != nullptr;
    float bias = 0.f, bsc = 0.f, bsh = 0.f, bmu = 0.f, bis = 0.f;
    if (!PRO) {
        bias = (p.bias && vn) ? p.bias[n] : 0.f;
        if (bnb && vn) { bsc = p.bnb_scale[n]; bsh = p.bnb_shift[n]; bmu = p.bnb_mean[n]; bis = p.bnb_invstd[n]; }
    }
    // (not in the variant with a BatchNorm prologue — the forward launches: it sits at 128 registers, and ten more are three waves per
    // SIMD instead of four, one 512-thread workgroup per CU instead of two: hg2 +0.07 ms.  The data-gradient launches — mask operand and
    // four BatchNorm-backward vectors in the epilogue — are the ones without a prologue)
    float r1v[2] = {0.f, 0.f};
    if (!PRO) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int mo = mtile * 32 + rg + 16 * j;
            if (vn && mo < p.M && p.res1) r1v[j] = p.res1[(size_t)mo * p.Cout + n];
        }
    }
    if (c0 < c1) {
        // two chunks in flight beside the one being multiplied; three register sets in rotation (no copies)
        Frag f0 = load_next(), f1 = load_next(), f2;
        for (int ch = c0;;) {
            f2 = load_next(); mma(f0); if (++ch >= c1) break;
            f0 = load_next(); mma(f1); if (++ch >= c1) break;
            f1 = load_next(); mma(f2); if (++ch >= c1) break;
        }
    }
    if (PRO) __syncthreads();                       // every wave is done with the vectors in `part`
    // partial tiles -> LDS (C/D layout: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5))
#pragma unroll
    for (int e = 0; e < 16; ++e) part[wave][(e & 3) + 8 * (e >> 2) + 4 * h][i] = acc[e];
    __syncthreads();
    if (PRO) {
        bias = (p.bias && vn) ? p.bias[n] : 0.f;
        if (bnb && vn) { bsc = p.bnb_scale[n]; bsh = p.bnb_shift[n]; bmu = p.bnb_mean[n]; bis = p.bnb_invstd[n]; }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = rg + 16 * j;
        const int mo = mtile * 32 + row;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += part[w][row][col];
        if (vn && mo < p.M) {
            const size_t o = (size_t)mo * p.Cout + n;
            if (bnb) {
                const float xv = PRO ? p.res1[o] : r1v[j];
                if (p.bnb_relu && fmaf(xv, bsc, bsh) <= 0.f) v = 0.f;
                p.y[o] = v;
                s1 += v;
                s2 = fmaf(v, (xv - bmu) * bis, s2);
            } else {
                v += bias + (PRO ? (p.res1 ? p.res1[o] : 0.f) : r1v[j]) + (p.res2 ? p.res2[o] : 0.f);
                p.y[o] = v;
                s1 += v;
                s2 = fmaf(v, v, s2);
            }
        }
    }
    if (p.stats) {
        __syncthreads();                             // every thread has read its part of `part`
        float* red = &part[0][0][0];                 // [16][32][2]
        red[(rg * 32 + col) * 2 + 0] = s1;
        red[(rg * 32 + col) * 2 + 1] = s2;
        __syncthreads();
        if (tid < 32 && vn) {
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int w = 0; w < 16; ++w) { a0 += red[(w * 32 + tid) * 2 + 0]; a1 += red[(w * 32 + tid) * 2 + 1]; }
            tail_store(p.stats + ((size_t)mtile * 2 + 0) * p.Cout + n, a0);
            tail_store(p.stats + ((size_t)mtile * 2 + 1) * p.Cout + n, a1);
        }
    }
}

template <bool PRO, int CW>
__global__ __launch_bounds__(512) void conv_ksplit_kernel(ConvP p) {
    __shared__ __attribute__((aligned(16))) float part[8][32][33];
    conv_ksplit_body<PRO, CW>(p, part);
}

// rows up to which the K-split kernel replaces the 32 x 128 tiling (measured crossover: 2048)
static long ksplit_rows() {
    static long v = -1;
    if (v < 0) {
        const char* e = getenv("DSNT_X_KSPLIT_ROWS");        // A/B only (tools/ab_env.sh)
        v = e ? atol(e) : 2048;
    }
    return v;
}

// fp32 path only, <= 256 input channels, <= 128 KB of partial sums: what every workgroup re-reads in its prologue
static bool conv_fwd_pro_ok(const dsnt_conv_geom* g, int tiles, int C) {
    return g && C == g->Cin && C <= 256 && C % 4 == 0 && tiles > 0 && (long)tiles * C <= 16384;
}
extern "C" int dsnt_conv_fwd_pro_ok(const dsnt_conv_geom* g, int tiles, int C) { return conv_fwd_pro_ok(g, tiles, C) ? 1 : 0; }

// (conv_split.h) what dsnt_conv_fwd* and dsnt_conv_fwd_bf16x6* / _f16x3* check and fill alike; the order of the checks is part of the ABI
int conv_fill(ConvP& p, const char* who, const float* x, const void* w, bool planes, int64_t plane_stride, const float* bias,
              float* y, const float* in_scale, const float* in_shift, int in_relu, const float* res1, const float* res2,
              float* stats_partial, const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail) {
    if (int e = conv_check_geom(g, who)) return e;
    char who_ex[64];
    snprintf(who_ex, sizeof(who_ex), "%s_ex", who);
    DSNT_REQUIRE(!bnb || (bnb->x && bnb->scale && bnb->shift && bnb->mean && bnb->invstd &&
                          stats_partial && !res1 && !res2 && !bias), DSNT_ERR_ARG,
                 "%s: the batch-norm-backward epilogue needs x/scale/shift/mean/invstd and "
                 "stats_partial, and excludes bias/residuals", who_ex);
    DSNT_REQUIRE(x && w && y, DSNT_ERR_ARG, "%s: null tensor", who);
    DSNT_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), DSNT_ERR_ARG,
                 "%s: in_scale/in_shift must be given together", who);
    DSNT_REQUIRE(!planes || dsnt_conv_bf16x6_ok(g), DSNT_ERR_SHAPE,
                 "%s: geometry not supported (need Cin %% 16 == 0, <= 16 taps, < 2 GiB)", who);
    DSNT_REQUIRE(dsnt_aligned16(x) && dsnt_aligned16(w) && (!in_scale || dsnt_aligned16(in_scale)) &&
                 (!in_shift || dsnt_aligned16(in_shift)), DSNT_ERR_ALIGN,
                 "%s: x/w/scale/shift must be 16-byte aligned", who);
    DSNT_REQUIRE(!planes || (plane_stride >= (int64_t)g->Cout * g->R * g->S * g->Cin && plane_stride % 8 == 0 &&
                             (2 * plane_stride + (int64_t)g->Cout * g->R * g->S * g->Cin) * 2 < (1LL << 31)), DSNT_ERR_SHAPE,
                 "%s: bad plane stride %lld", who, (long long)plane_stride);
    p.x = x; p.bias = bias; p.y = y; p.in_scale = in_scale; p.in_shift = in_shift;
    p.w = planes ? nullptr : (const float*)w;
    p.wq = planes ? (const unsigned short*)w : nullptr; p.wq_stride = planes ? plane_stride : 0;
    p.res1 = res1; p.res2 = res2; p.stats = stats_partial; p.in_relu = in_relu;
    p.bnb_scale = p.bnb_shift = p.bnb_mean = p.bnb_invstd = nullptr; p.bnb_relu = 0;
    p.a_bound = p.w_bound = nullptr;
    p.ap_y = p.ap_scale = p.ap_mean = p.ap_invstd = p.ap_coef = nullptr; p.ap_out = nullptr;
    if (bnb) {
        p.res1 = bnb->x; p.bnb_scale = bnb->scale; p.bnb_shift = bnb->shift;
        p.bnb_mean = bnb->mean; p.bnb_invstd = bnb->invstd; p.bnb_relu = bnb->relu;
    }
    if (int e = out_bounds_fill(p.tail, tail, who_ex)) return e;
    DSNT_REQUIRE(!(p.tail.amax_bn && bnb), DSNT_ERR_ARG, "%s: dsnt_out_bounds.amax_bn excludes the batch-norm-backward epilogue", who_ex);
    memset(&p.pro, 0, sizeof(p.pro));
    conv_geom_fill(p, g);
    return DSNT_OK;
}

static int conv_fwd_impl(const float* x, const float* w, const float* bias, float* y,
                         const float* in_scale, const float* in_shift, int in_relu,
                         const float* res1, const float* res2, float* stats_partial,
                         const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* g_bnb, const dsnt_out_bounds* g_tail,
                         void* stream, const dsnt_bn_prologue* g_pro = nullptr) {
    ConvP p;
    if (int e = conv_fill(p, "dsnt_conv_fwd", x, w, false, 0, bias, y, in_scale, in_shift, in_relu, res1, res2, stats_partial, g,
                          g_bnb, g_tail)) return e;
    if (g_pro) {
        DSNT_REQUIRE(g_pro->partial && g_pro->mean && g_pro->invstd && g_pro->scale && g_pro->shift && g_pro->M > 0 &&
                     conv_fwd_pro_ok(g, g_pro->tiles, g_pro->C), DSNT_ERR_ARG,
                     "dsnt_conv_fwd_pro: incomplete dsnt_bn_prologue, or more than 256 channels / 128 KB of partial sums");
        DSNT_REQUIRE((g_pro->running_mean == nullptr) == (g_pro->running_var == nullptr), DSNT_ERR_ARG,
                     "dsnt_conv_fwd_pro: running_mean/var must be given together");
        DSNT_REQUIRE(dsnt_aligned16(g_pro->scale) && dsnt_aligned16(g_pro->shift), DSNT_ERR_ALIGN, "dsnt_conv_fwd_pro: alignment");
        p.pro.partial = g_pro->partial; p.pro.tiles = g_pro->tiles; p.pro.C = g_pro->C;
        p.pro.invM = 1.0 / (double)g_pro->M;
        p.pro.unbias = g_pro->M > 1 ? (double)g_pro->M / (double)(g_pro->M - 1) : 1.0;
        p.pro.gamma = g_pro->gamma; p.pro.beta = g_pro->beta; p.pro.rmean = g_pro->running_mean; p.pro.rvar = g_pro->running_var;
        p.pro.momentum = g_pro->momentum; p.pro.eps = g_pro->eps;
        p.pro.mean = g_pro->mean; p.pro.invstd = g_pro->invstd; p.pro.scale = g_pro->scale; p.pro.shift = g_pro->shift;
    }
    int BM, BN;
    pick_cfg(g, BM, BN);
    p.mtiles = (p.M + BM - 1) / BM; p.ntiles = (p.Cout + BN - 1) / BN;
    hipStream_t st = (hipStream_t)stream;
    const bool pro = in_scale != nullptr;
    if (BM == 32 && p.M <= ksplit_rows() && p.Cin % 8 == 0 && (size_t)p.N * p.H * p.W * p.Cin * 4u < (1ull << 31) &&
        (size_t)p.Cout * p.K * 4u < (1ull << 31) && !p.tail.amax && !p.tail.amax_bn &&        // (the K-split epilogue has no amax)
        (!pro || p.Cin <= 4096)) {
        const int grid = p.mtiles * ((p.Cout + 31) / 32);
        // (KS_CW: experiments only)
#ifndef KS_CW
#define KS_CW 16
#endif
        if (p.Cin % KS_CW == 0) {
            if (pro) DSNT_LAUNCH((conv_ksplit_kernel<true, KS_CW>), dim3(grid), dim3(512), 0, st, p);
            else DSNT_LAUNCH((conv_ksplit_kernel<false, KS_CW>), dim3(grid), dim3(512), 0, st, p);
        } else if (pro) DSNT_LAUNCH((conv_ksplit_kernel<true, 8>), dim3(grid), dim3(512), 0, st, p);
        else DSNT_LAUNCH((conv_ksplit_kernel<false, 8>), dim3(grid), dim3(512), 0, st, p);
    } else if (BM == 128 && BN == 128) launch_fwd<2, 2, 2, 2>(p, pro, st);
    else if (BM == 128 && BN == 64) launch_fwd<2, 2, 2, 1>(p, pro, st);
    else if (BM == 128 && BN == 32) launch_fwd<4, 1, 1, 1>(p, pro, st);
    else launch_fwd<1, 4, 1, 1>(p, pro, st);
    DSNT_CHECK_LAUNCH("dsnt_conv_fwd");
}

extern "C" int dsnt_conv_fwd(const float* x, const float* w, const float* bias, float* y,
                             const float* in_scale, const float* in_shift, int in_relu,
                             const float* res1, const float* res2, float* stats_partial,
                             const dsnt_conv_geom* g, void* stream) {
    return conv_fwd_impl(x, w, bias, y, in_scale, in_shift, in_relu, res1, res2, stats_partial, g, nullptr, nullptr, stream);
}

extern "C" int dsnt_conv_fwd_ex(const float* x, const float* w, const float* bias, float* y,
                                const float* in_scale, const float* in_shift, int in_relu,
                                const float* res1, const float* res2, float* stats_partial,
                                const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail,
                                void* stream) {
    return conv_fwd_impl(x, w, bias, y, in_scale, in_shift, in_relu, res1, res2, stats_partial, g, bnb, tail, stream);
}

extern "C" int dsnt_conv_fwd_pro(const float* x, const float* w, const float* bias, float* y, const dsnt_bn_prologue* pro,
                                 int in_relu, const float* res1, const float* res2, float* stats_partial,
                                 const dsnt_conv_geom* g, const dsnt_out_bounds* tail, void* stream) {
    DSNT_REQUIRE(pro, DSNT_ERR_ARG, "dsnt_conv_fwd_pro: null dsnt_bn_prologue");
    return conv_fwd_impl(x, w, bias, y, pro->scale, pro->shift, in_relu, res1, res2, stats_partial, g, nullptr, tail, stream, pro);
}
