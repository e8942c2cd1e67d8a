// Implicit-GEMM weight gradients of the convolutions: the fp32-MFMA and the role-split bf16x6 / fp16x3 kernels over m-slabs
// (deterministic, no atomics) with the grouped form of the latter, behind the plan / launch / descriptor interface of wgrad.h.
// The dispatch that reaches them (and the halo, 1x1 and stem kernels instead, where those apply): conv_wgrad.hip; the slab
// reduction that follows: wgrad_reduce.hip.
#include "conv_split.h"
#include "wgrad.h"
#include <string.h>

// GEMM view: D[k][n] = sum_m A[m][k] * G[m][n], tile 128(k) x 128(n),
// m consumed 32 rows per step.  Both LDS tiles are [32 m][128] row-major; the MFMA operands are
// read with ds_read_b32: lane (i = l&31, mm = l>>5) takes A[m = 2t+mm][k = i] and
// G[m = 2t+mm][n = i] — consecutive lanes, consecutive banks.
struct WgradP {
    const float* x; const float* in_scale; const float* in_shift; const float* dy;
    float* ws;  // [splits][Cout][K] slabs, then [splits][Cout] bias partials
    int in_relu;
    int N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil;
    int M, K, ktiles, ntiles, splits, rows_per_split;
    // fp16x3: bound slots of the A operand (after its BN+ReLU prologue) and of dy; null on the bf16x6 path
    const float* a_bound; const float* g_bound;
};

#define WPITCH 132

// VALU diet (fp32 MFMA and VALU are serialised on gfx950): each thread's filter tap / channel
// chunk is fixed for the whole kernel, rows advance by 32 per step with incremental (n, oh, ow)
// carries instead of divisions, loads are range-checked buffer loads (invalid rows / padded taps
// point out of range and come back as zeros), two register sets keep two steps of loads in flight.
template <bool PRO>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(WgradP p) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float As[2][32][WPITCH];
    __shared__ __attribute__((aligned(16))) float Gs[2][32][WPITCH];

    int bid;
    xcd_remap(blockIdx.x, gridDim.x, bid);
    const int ktile = bid % p.ktiles; bid /= p.ktiles;
    const int ntile = bid % p.ntiles;
    const int split = bid / p.ntiles;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1;   // wave owns k rows [64wk,64wk+64), n cols [64wn, ..)
    const int li = lane & 31, lm = lane >> 5;
    const int lrow = tid >> 5, cc = tid & 31;  // loader: row lrow + 8i, float4 column cc

    const int k0 = ktile * 128 + cc * 4;
    const bool vk = k0 < p.K;
    const int tap = k0 / p.Cin, c = k0 - tap * p.Cin;
    const int r = tap / p.S, s = tap - r * p.S;
    const int dh = r * p.dil - p.pad, dw = s * p.dil - p.pad;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (PRO && vk) {
        sc = *reinterpret_cast<const float4*>(p.in_scale + c);
        sh = *reinterpret_cast<const float4*>(p.in_shift + c);
    }
    const int n0 = ntile * 128 + cc * 4;
    const bool vn = n0 < p.Cout;

    const int m_begin = split * p.rows_per_split;
    const int m_end = min(p.M, m_begin + p.rows_per_split);
    const int HoWo = p.Ho * p.Wo;
    const int adv_h = 32 / p.Wo, adv_w = 32 - adv_h * p.Wo;     // scalars: 32 rows = adv_h rows + adv_w cols

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x), 0, (int)((size_t)p.N * p.H * p.W * p.Cin * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.dy), 0, (int)((size_t)p.M * p.Cout * 4u), 0x00020000);
    const unsigned OOB = 0xF0000000u;

    // per-row state of this thread's four rows
    int rn[4], roh[4], row_[4], rm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m_begin + lrow + 8 * i;
        rm[i] = m;
        const int mm = m < p.M ? m : 0;
        rn[i] = mm / HoWo;
        const int rem = mm - rn[i] * HoWo;
        roh[i] = rem / p.Wo;
        row_[i] = rem - roh[i] * p.Wo;
    }
    struct Stage { u32x4 a[4], g[4]; unsigned ok; };
    Stage S0, S1;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    // issue the loads of the current rows, then advance the rows by 32
    auto gload = [&](Stage& st) {
        st.ok = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool vm = rm[i] < m_end;
            const int ih = roh[i] * p.stride + dh, iw = row_[i] * p.stride + dw;
            const bool oka = vm && vk && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            const unsigned offa = oka ? (unsigned)(((rn[i] * p.H + ih) * p.W + iw) * p.Cin + c) * 4u : OOB;
            st.a[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, offa, 0, 0);
            const unsigned offg = (vm && vn) ? (unsigned)(rm[i] * p.Cout + n0) * 4u : OOB;
            st.g[i] = __builtin_amdgcn_raw_buffer_load_b128(gr, offg, 0, 0);
            st.ok |= (oka ? 1u : 0u) << i;
            // advance
            rm[i] += 32;
            row_[i] += adv_w;
            roh[i] += adv_h;
            if (row_[i] >= p.Wo) { row_[i] -= p.Wo; roh[i] += 1; }
            while (roh[i] >= p.Ho) { roh[i] -= p.Ho; rn[i] += 1; }
        }
    };
    auto lstore = [&](const Stage& st, int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 va = make_float4(__uint_as_float(st.a[i].x), __uint_as_float(st.a[i].y),
                                    __uint_as_float(st.a[i].z), __uint_as_float(st.a[i].w));
            const float4 vg = make_float4(__uint_as_float(st.g[i].x), __uint_as_float(st.g[i].y),
                                          __uint_as_float(st.g[i].z), __uint_as_float(st.g[i].w));
            if (PRO) {
                va.x = fmaf(va.x, sc.x, sh.x); va.y = fmaf(va.y, sc.y, sh.y);
                va.z = fmaf(va.z, sc.z, sh.z); va.w = fmaf(va.w, sc.w, sh.w);
                if (p.in_relu) {
                    va.x = fmaxf(va.x, 0.f); va.y = fmaxf(va.y, 0.f);
                    va.z = fmaxf(va.z, 0.f); va.w = fmaxf(va.w, 0.f);
                }
                const bool ok = (st.ok >> i) & 1u;     // branch-free (see the forward loader)
                va.x = ok ? va.x : 0.f; va.y = ok ? va.y : 0.f; va.z = ok ? va.z : 0.f; va.w = ok ? va.w : 0.f;
            }
            *reinterpret_cast<float4*>(&As[buf][lrow + 8 * i][cc * 4]) = va;   // OOB loads are zeros
            *reinterpret_cast<float4*>(&Gs[buf][lrow + 8 * i][cc * 4]) = vg;
            bsum.x += vg.x; bsum.y += vg.y; bsum.z += vg.z; bsum.w += vg.w;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    auto compute = [&](int buf) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            float fa[2], fb[2];
            fa[0] = As[buf][2 * t + lm][wk * 64 + li];
            fa[1] = As[buf][2 * t + lm][wk * 64 + 32 + li];
            fb[0] = Gs[buf][2 * t + lm][wn * 64 + li];
            fb[1] = Gs[buf][2 * t + lm][wn * 64 + 32 + li];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
    };

    const int nsteps = (m_end - m_begin + 31) / 32;
    // S0 holds step 0 (then 2, 4, ...), S1 holds step 1 (3, 5, ...): two steps of loads in flight
    // unconditional on purpose (hipcc's vmcnt bookkeeping is exact only on straight-line code, see the
    // forward loader): rows past m_end load nothing (out-of-range buffer offsets) and store zeros
    gload(S0);
    gload(S1);
    lstore(S0, 0);
    gload(S0);
    __syncthreads();
    int st = 0;
    for (; st + 1 < nsteps; st += 2) {
        compute(0);
        __builtin_amdgcn_sched_barrier(0);
        lstore(S1, 1);
        gload(S1);
        __syncthreads();
        compute(1);
        __builtin_amdgcn_sched_barrier(0);
        lstore(S0, 0);
        gload(S0);
        __syncthreads();
    }
    if (st < nsteps) compute(0);

    // slab store: ws[split][n][k], D row = k (regs, 4 consecutive), D col = n (lane)
    float* slab = p.ws + (size_t)split * p.Cout * p.K;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int n = ntile * 128 + wn * 64 + b * 32 + li;
        if (n >= p.Cout) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = ktile * 128 + wk * 64 + a * 32 + 8 * q + 4 * lm;
                if (k < p.K) {
                    float4 v = make_float4(acc[a][b][4 * q + 0], acc[a][b][4 * q + 1],
                                           acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]);
                    *reinterpret_cast<float4*>(slab + (size_t)n * p.K + k) = v;
                }
            }
        }
    }
    // bias partial: column sums of this split's dY rows (only the ktile-0 blocks)
    if (ktile == 0) {
        float* red = &As[0][0][0];  // [8][128] floats
        __syncthreads();
        *reinterpret_cast<float4*>(red + lrow * 128 + cc * 4) = bsum;
        __syncthreads();
        if (tid < 128) {
            const int n = ntile * 128 + tid;
            if (n < p.Cout) {
                float t = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) t += red[j * 128 + tid];
                p.ws[(size_t)p.splits * p.Cout * p.K + (size_t)split * p.Cout + n] = t;
            }
        }
    }
}

// bf16x6 weight gradient: D[k][n] = sum_m A[m][k] G[m][n] on the bf16 matrix cores (see the
// forward bf16x6 kernel for the numerics).  The reduction index of the MFMA is m, so both LDS tiles
// are stored transposed ([k][m] and [n][m], m contiguous): a loader thread owns a 4(m) x 4(k or n)
// block, loads four rows, applies BN+ReLU / zero padding (A only), splits and packs pairs of ROWS with
// v_cvt_pk_bf16_f32, i.e. the transpose costs no extra instruction.  128 threads stage A, 128 stage G;
// waves 0..3 run the MFMAs (64 x 64 of the 128 x 128 tile each), one barrier per 16 rows of m.
//
// The kernel is bound by the loaders' VALU work (a SIMD issues either an MFMA or a VALU instruction:
// DESIGN.md "issue starvation"), so the two loader kinds are separate straight-line instantiations:
// the G waves only split (out-of-range buffer loads already return zeros), the A waves fold ReLU and
// the zero-padding select into one v_med3_f32 against per-row bounds, and the split itself runs on
// plain (unpacked) fp32 ops (split4).
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <bool PRO, bool IS_A, bool F16>
__device__ __forceinline__ void wgrad6_loader(const WgradP& p, __bf16* T, const int ltid, const int ktile,
                                              const int ntile, const int m_begin, const int m_end,
                                              const int nsteps, f32x2& bs0, f32x2& bs1) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr int NPL = F16 ? 2 : 3;
    // fp16x3: power-of-two operand scale from the bound slots (A: folded into the BN vectors below; dY: one multiply)
    const float sop = F16 ? pow2_scale(bound64(IS_A ? p.a_bound : p.g_bound)) : 1.f;
    // 4-wide column chunk q, 4-row block mb.  mb varies fastest: a 16-lane store group then spans
    // 4 chunks x 4 blocks (2-way bank conflicts; q fastest would be 8-way with the 48-byte pitch)
    const int mb = ltid & 3, q = (ltid >> 2) & 31;
    const unsigned OOB = 0xF0000000u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(IS_A ? p.x : p.dy), 0,
        IS_A ? (int)((size_t)p.N * p.H * p.W * p.Cin * 4u) : (int)((size_t)p.M * p.Cout * 4u), 0x00020000);
    // A side: fixed tap / channel chunk
    const int k0 = ktile * 128 + q * 4;
    const bool vk = k0 < p.K;
    const int tap = k0 / p.Cin, c = k0 - tap * p.Cin;
    const int r = tap / p.S, s_ = tap - r * p.S;
    const int dh = r * p.dil - p.pad, dw = s_ * p.dil - p.pad;
    f32x2 sc0 = {1.f, 1.f}, sc1 = {1.f, 1.f}, sh0 = {0.f, 0.f}, sh1 = {0.f, 0.f};
    if (PRO && IS_A && vk) {
        const float4 a = *reinterpret_cast<const float4*>(p.in_scale + c);
        const float4 b = *reinterpret_cast<const float4*>(p.in_shift + c);
        sc0 = (f32x2){a.x, a.y}; sc1 = (f32x2){a.z, a.w};
        sh0 = (f32x2){b.x, b.y}; sh1 = (f32x2){b.z, b.w};
        if (F16) { sc0 *= sop; sc1 *= sop; sh0 *= sop; sh1 *= sop; }
    }
    // ReLU and the padding select as one median: valid rows clamp to [lo, +inf) with lo = 0 (ReLU) or
    // -inf (no ReLU), invalid rows to [0, 0]
    const float lo_valid = (PRO && IS_A && p.in_relu) ? 0.f : -__builtin_inff();
    // G side
    const int n0 = ntile * 128 + q * 4;
    const bool vn = n0 < p.Cout;
    // first row of this thread's 4-row block (Wo % 4 == 0: the 4 rows share n and oh)
    const int HoWo = p.Ho * p.Wo;
    int rm = m_begin + mb * 4;
    const int mm0 = rm < p.M ? rm : 0;
    int rn = mm0 / HoWo;
    int roh = (mm0 - rn * HoWo) / p.Wo;
    int row_ = mm0 - rn * HoWo - roh * p.Wo;
    const int adv_h = 16 / p.Wo, adv_w = 16 - adv_h * p.Wo;
    struct Stage { u32x4 v[4]; unsigned ok; };
    Stage S0, S1;
    auto gload = [&](Stage& st) {
        st.ok = 0;
        if (IS_A) {
            const int ih = roh * p.stride + dh;
            const bool vrow = vk && ih >= 0 && ih < p.H;
            const int base = ((rn * p.H + ih) * p.W) * p.Cin + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iw = (row_ + j) * p.stride + dw;
                const bool ok = (rm + j) < m_end && vrow && iw >= 0 && iw < p.W;
                const unsigned off = (unsigned)(base + iw * p.Cin) * 4u;
                st.v[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off : OOB, 0, 0);
                st.ok |= (ok ? 1u : 0u) << j;
            }
            row_ += adv_w; roh += adv_h;
            if (row_ >= p.Wo) { row_ -= p.Wo; roh += 1; }
            // 16 rows cross at most one image boundary when an image has >= 16 pixels (branch-free); tiny maps loop
            if (HoWo >= 16) { const bool wrap = roh >= p.Ho; roh = wrap ? roh - p.Ho : roh; rn = wrap ? rn + 1 : rn; }
            else while (roh >= p.Ho) { roh -= p.Ho; rn += 1; }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = (rm + j) < m_end && vn;
                const unsigned off = (unsigned)((rm + j) * p.Cout + n0) * 4u;
                st.v[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off : OOB, 0, 0);
            }
        }
        rm += 16;
    };
    auto lstore = [&](const Stage& st, int buf) {
        f32x2 v0[4], v1[4];      // (x, y) and (z, w) of the four rows
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v0[j] = (f32x2){__uint_as_float(st.v[j].x), __uint_as_float(st.v[j].y)};
            v1[j] = (f32x2){__uint_as_float(st.v[j].z), __uint_as_float(st.v[j].w)};
            if (PRO && IS_A) {
                v0[j].x = fmaf(v0[j].x, sc0.x, sh0.x); v0[j].y = fmaf(v0[j].y, sc0.y, sh0.y);
                v1[j].x = fmaf(v1[j].x, sc1.x, sh1.x); v1[j].y = fmaf(v1[j].y, sc1.y, sh1.y);
                const bool ok = (st.ok >> j) & 1u;
                const float lo = ok ? lo_valid : 0.f, hi = ok ? __builtin_inff() : 0.f;
                v0[j].x = __builtin_amdgcn_fmed3f(v0[j].x, lo, hi); v0[j].y = __builtin_amdgcn_fmed3f(v0[j].y, lo, hi);
                v1[j].x = __builtin_amdgcn_fmed3f(v1[j].x, lo, hi); v1[j].y = __builtin_amdgcn_fmed3f(v1[j].y, lo, hi);
            }
            if (!IS_A) { bs0.x += v0[j].x; bs0.y += v0[j].y; bs1.x += v1[j].x; bs1.y += v1[j].y; }
        }
        __bf16* base = T + ((size_t)(buf * NPL) * 128 + q * 4) * PITCH6 + mb * 4;
        // component e of the four rows -> LDS row (q*4 + e), columns mb*4 .. mb*4+3, three planes
#define SPLIT_COL(E, V, COMP)                                                                        \
        {                                                                                            \
            uint2 q1, q2, q3;                                                                        \
            float4 c4 = make_float4(V[0].COMP, V[1].COMP, V[2].COMP, V[3].COMP);                     \
            __bf16* d = base + (E) * PITCH6;                                                         \
            if (F16) {                                                                               \
                if (!(PRO && IS_A)) { c4.x *= sop; c4.y *= sop; c4.z *= sop; c4.w *= sop; }          \
                split4h(c4, q1, q2);                                                                 \
                *reinterpret_cast<uint2*>(d) = q1;                                                   \
                *reinterpret_cast<uint2*>(d + 128 * PITCH6) = q2;                                    \
            } else {                                                                                 \
                split4(c4, q1, q2, q3);                                                              \
                *reinterpret_cast<uint2*>(d) = q1;                                                   \
                *reinterpret_cast<uint2*>(d + 128 * PITCH6) = q2;                                    \
                *reinterpret_cast<uint2*>(d + 2 * 128 * PITCH6) = q3;                                \
            }                                                                                        \
        }
        SPLIT_COL(0, v0, x) SPLIT_COL(1, v0, y) SPLIT_COL(2, v1, x) SPLIT_COL(3, v1, y)
#undef SPLIT_COL
    };
    // unconditional (see the forward loader): rows past m_end load nothing and store zeros
    gload(S0);
    gload(S1);
    lstore(S0, 0);
    gload(S0);
    __syncthreads();
    int s = 0;
    for (; s + 1 < nsteps; s += 2) {
        lstore(S1, 1);
        gload(S1);
        __syncthreads();
        lstore(S0, 0);
        gload(S0);
        __syncthreads();
    }
    if (s < nsteps) __syncthreads();
}

template <bool PRO, bool F16 = false>
__device__ __forceinline__ void wgrad6_body(const WgradP& p, int bid, float* smem) {
    constexpr int NPL = F16 ? 2 : 3;
    __bf16* At = reinterpret_cast<__bf16*>(smem);            // [2][NPL][128][PITCH6]
    __bf16* Gt = At + 2 * NPL * 128 * PITCH6;                // [2][NPL][128][PITCH6]

    const int ktile = bid % p.ktiles; bid /= p.ktiles;
    const int ntile = bid % p.ntiles;
    const int split = bid / p.ntiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int m_begin = split * p.rows_per_split;
    const int m_end = min(p.M, m_begin + p.rows_per_split);
    const int nsteps = (m_end - m_begin + 15) / 16;

    f32x2 bs0 = {0.f, 0.f}, bs1 = {0.f, 0.f};

    if (wave >= 6) {
        wgrad6_loader<PRO, false, F16>(p, Gt, tid - 384, ktile, ntile, m_begin, m_end, nsteps, bs0, bs1);
    } else if (wave >= 4) {
        wgrad6_loader<PRO, true, F16>(p, At, tid - 256, ktile, ntile, m_begin, m_end, nsteps, bs0, bs1);
    } else {
        // ------------------------------------------------------------------ MFMA waves
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
        const int wk = wave >> 1, wn = wave & 1;
        struct Frag { bf16x8 a[2][3], b[2][3]; };
        Frag F;
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            const int buf = s & 1;
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    F.a[t][pl] = *reinterpret_cast<const bf16x8*>(
                        At + ((size_t)(buf * NPL + pl) * 128 + wk * 64 + t * 32 + lr) * PITCH6 + 8 * lh);
                    F.b[t][pl] = *reinterpret_cast<const bf16x8*>(
                        Gt + ((size_t)(buf * NPL + pl) * 128 + wn * 64 + t * 32 + lr) * PITCH6 + 8 * lh);
                }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) mma_split<F16>(acc[a][b], F.a[a], F.b[b]);
            __syncthreads();
        }
        // slab store: ws[split][n][k], D row = k (regs, 4 consecutive), D col = n (lane)
        // (fp16x3: the accumulators hold (A s_a)^T (dY s_g); both scales are powers of two, undone exactly)
        const float osc = F16 ? 1.f / (pow2_scale(bound64(p.a_bound)) * pow2_scale(bound64(p.g_bound))) : 1.f;
        float* slab = p.ws + (size_t)split * p.Cout * p.K;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = ntile * 128 + wn * 64 + b * 32 + lr;
            if (n >= p.Cout) continue;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {
                    const int k = ktile * 128 + wk * 64 + a * 32 + 8 * qq + 4 * lh;
                    if (k < p.K)
                        *reinterpret_cast<float4*>(slab + (size_t)n * p.K + k) =
                            make_float4(acc[a][b][4 * qq + 0] * osc, acc[a][b][4 * qq + 1] * osc,
                                        acc[a][b][4 * qq + 2] * osc, acc[a][b][4 * qq + 3] * osc);
                }
        }
    }
    // bias partial: column sums of this split's dY rows (G loader threads of the ktile-0 blocks)
    if (ktile == 0) {
        float* red = smem;   // [4][128] floats
        __syncthreads();
        if (wave >= 6) {
            const int ltid = tid - 384;
            *reinterpret_cast<float4*>(red + (ltid & 3) * 128 + ((ltid >> 2) & 31) * 4) =
                make_float4(bs0.x, bs0.y, bs1.x, bs1.y);
        }
        __syncthreads();
        if (tid < 128) {
            const int n = ntile * 128 + tid;
            if (n < p.Cout)
                p.ws[(size_t)p.splits * p.Cout * p.K + (size_t)split * p.Cout + n] =
                    red[tid] + red[128 + tid] + red[256 + tid] + red[384 + tid];
        }
    }
}

template <bool PRO, bool F16 = false>
__global__ __launch_bounds__(512, 2) void conv_wgrad_bf16x6_kernel(WgradP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // the k-tiles (filter taps) and n-tiles of one split read the same rows of x and dy: keep them in one
    // XCD (one L2) instead of dealing them round-robin over the eight
    int bid;
    xcd_remap(blockIdx.x, gridDim.x, bid);
    wgrad6_body<PRO, F16>(p, bid, smem);
}

// Grouped launch: blockIdx.y picks one of many convolutions from a device table of WgradP descriptors
// (dsnt_conv_wgrad_desc), blockIdx.x is the block within it.  The ~50 weight gradients of the 16x16 ... 4x4
// hourglass levels have 4 ... 288 workgroups each and take 25-55 us apiece as separate launches (a serial
// chain of 16-row steps per workgroup, nothing to overlap with); nothing downstream in backward needs them,
// so the engine defers them to the end of their parameter bucket and runs them side by side in ONE launch.
__global__ __launch_bounds__(512, 2) void conv_wgrad_bf16x6_group_kernel(const WgradP* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WgradP p = table[blockIdx.y];
    const int nblk = p.ktiles * p.ntiles * p.splits;
    if ((int)blockIdx.x >= nblk) return;
    if (p.a_bound) wgrad6_body<true, true>(p, blockIdx.x, smem);        // workgroup-uniform: fp16x3 descriptors
    else wgrad6_body<true, false>(p, blockIdx.x, smem);
}

WgGemmPlan dsnt_wgg_plan(const dsnt_conv_geom* g) {
    WgGemmPlan pl;
    memset(&pl, 0, sizeof(pl));
    const long M = (long)g->N * g->Ho * g->Wo;
    const int K = g->R * g->S * g->Cin;
    if (M < 1 || K < 1 || g->Cout < 1) return pl;      // (conv_check_geom refuses these; a query gets zero slabs, not a division by zero)
    const int ktiles = (K + 127) / 128;
    const int ntiles = (g->Cout + 127) / 128;
    // 256 workgroups = one per CU: these launches run at one workgroup per CU beside the dependency chain anyway
    // (DSNT_WGRAD_SHARE_CHIP), and half as many splits are half the slab traffic (512 measured +0.2 ms per hg2 step)
    const long target = 256;
    long want = target / (ktiles * ntiles);
    if (want < 1) want = 1;
    long max_splits = (M + 255) / 256;         // at least 8 steps of 32 rows per split
    if (max_splits < 1) max_splits = 1;
    long sp = want < max_splits ? want : max_splits;
    long rows = (M + sp - 1) / sp;
    rows = (rows + 31) / 32 * 32;
    sp = (M + rows - 1) / rows;
    pl.ktiles = ktiles; pl.ntiles = ntiles;
    pl.splits = (int)sp;
    pl.rows_per_split = (int)rows;
    return pl;
}

static void wgrad_fill(WgradP& p, const WgGemmPlan& pl, const float* x, const float* in_scale, const float* in_shift,
                       int in_relu, const float* dy, float* ws, const float* a_bound, const float* g_bound,
                       const dsnt_conv_geom* g) {
    memset(&p, 0, sizeof(p));
    p.a_bound = a_bound; p.g_bound = g_bound;
    p.x = x; p.in_scale = in_scale; p.in_shift = in_shift; p.dy = dy; p.ws = ws; p.in_relu = in_relu;
    conv_geom_fill(p, g);
    p.ktiles = pl.ktiles; p.ntiles = pl.ntiles; p.splits = pl.splits; p.rows_per_split = pl.rows_per_split;
}

// DSNT_WGRAD_SHARE_CHIP: the launch runs beside a dependency chain on another stream.  Its workgroups live as long as the
// kernel (one wave of ~2 per CU), and two of them fill a CU's registers: the chain's small kernels (a 16-workgroup BatchNorm
// finalise) then wait for the whole weight gradient to end — 150 us seen.  Asking for more than half of the LDS keeps it to
// ONE workgroup per CU and the other half of every CU free.
template <bool PRO, bool F16>
static void wgg_launch6(const WgradP& p, bool share, hipStream_t st) {
    const int share_lds = 88 * 1024;
    const int lds = share ? share_lds : 2 * 2 * (F16 ? 2 : 3) * 128 * PITCH6 * 2;     // fp16x3: two planes, 2/3 of the LDS
    DSNT_SET_MAX_LDS((conv_wgrad_bf16x6_kernel<PRO, F16>), share_lds);
    DSNT_LAUNCH((conv_wgrad_bf16x6_kernel<PRO, F16>), dim3(p.ktiles * p.ntiles * p.splits), dim3(512), lds, st, p);
}

void dsnt_wgg_launch(const WgGemmPlan& pl, bool bf16x6, const float* x, const float* in_scale, const float* in_shift,
                     int in_relu, const float* dy, float* ws, const float* a_bound, const float* g_bound,
                     const dsnt_conv_geom* g, hipStream_t st, bool share) {
    WgradP p;
    wgrad_fill(p, pl, x, in_scale, in_shift, in_relu, dy, ws, a_bound, g_bound, g);
    if (!bf16x6) {
        const int grid = p.ktiles * p.ntiles * p.splits;
        if (in_scale) DSNT_LAUNCH(conv_wgrad_kernel<true>, dim3(grid), dim3(256), 0, st, p);
        else DSNT_LAUNCH(conv_wgrad_kernel<false>, dim3(grid), dim3(256), 0, st, p);
    } else if (a_bound) {
        if (in_scale) wgg_launch6<true, true>(p, share, st);
        else wgg_launch6<false, true>(p, share, st);
    } else {
        if (in_scale) wgg_launch6<true, false>(p, share, st);
        else wgg_launch6<false, false>(p, share, st);
    }
}

int dsnt_wgg_desc_bytes(void) { return (int)sizeof(WgradP); }

int dsnt_wgg_desc(const float* x, const float* in_scale, const float* in_shift, int in_relu, const float* dy, float* ws,
                  const float* a_bound, const float* g_bound, const dsnt_conv_geom* g, void* desc_out) {
    WgradP p;
    wgrad_fill(p, dsnt_wgg_plan(g), x, in_scale, in_shift, in_relu, dy, ws, a_bound, g_bound, g);
    memcpy(desc_out, &p, sizeof(p));
    return p.ktiles * p.ntiles * p.splits;
}

void dsnt_wgg_launch_group(const void* table, int nconv, int max_blocks, hipStream_t st) {
    const int lds = 2 * 2 * 3 * 128 * PITCH6 * 2;
    DSNT_SET_MAX_LDS(conv_wgrad_bf16x6_group_kernel, lds);
    DSNT_LAUNCH(conv_wgrad_bf16x6_group_kernel, dim3(max_blocks, nconv), dim3(512), lds, st, (const WgradP*)table);
}
