// The epilogue shared by the tiled forward / data-gradient kernels (conv_f32.hip, conv_split6.hip): the accumulators go through
// LDS to row-major 16-byte accesses; bias, residuals or the BatchNorm-backward mask, the operand bounds of the output's
// consumers and the per-tile column statistics are applied on the way out.  Device code only (gfx950).
#pragma once
#include "conv_split.h"

// Shared epilogue of the forward / data-gradient kernels (fp32 and bf16x6 variants).
// HALO: the tile's 128 rows are an 8 x 16 patch of output pixels starting at row `mbase` (row r of the
// tile is output row mbase + (r >> 4) * W + (r & 15)) instead of 128 consecutive output rows.
template <int WM, int WN, int TM, int TN, bool HALO = false, int NT = 512>
__device__ __forceinline__ void conv_epilogue(const ConvP& p, f32x16 (&acc)[TM][TN], float* smem, int mtile,
                                              int ntile, int tid, int wave, int lane, int mbase = 0) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    // (odd patch rows are rotated by two pixels: tile row r holds pixel column (r + 14) & 15 there, which keeps
    // the 18-pixel halo pitch on the conflict-free ds_read_b128 bank pattern — see conv3x3_bf16x6_kernel)
    auto rowmap = [&](int row) {
        return HALO ? mbase + (row >> 4) * p.W + (((row & 15) + ((row >> 4) & 1) * 14) & 15) : mtile * BM + row;
    };
    const int lr = lane & 31, lh = lane >> 5;
    const int cw = wave & 3;
    const int wm = cw / WN, wn = cw % WN;
    // ---- epilogue.  The accumulators (C/D layout: col = lane&31, row = (reg&3) + 8*(reg>>2) +
    // 4*(lane>>5)) are transposed through LDS into row-major [BM][BN] so that bias / residual /
    // store run as 16-byte row-contiguous accesses, all loads issued before the first use.
    constexpr int CP = BN + 4;                 // C-tile pitch (floats)
    float* Cs = smem;                          // [BM][CP]; the main loop ended with a barrier
    if (wave < 4) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int col = (wn * TN + b) * 32 + lr;
                const int row0 = (wm * TM + a) * 32 + 4 * lh;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    Cs[(row0 + (e & 3) + 8 * (e >> 2)) * CP + col] = acc[a][b][e];
            }
    }
    __syncthreads();
    constexpr int CH = BN / 4;                 // float4 chunks per row
    constexpr int RPP = NT / CH;               // rows per pass
    constexpr int NPT = BM / RPP;              // passes
    constexpr int NP = NPT > 8 ? 8 : NPT;      // passes per group (bounds the residual registers)
    constexpr int NG = NPT / NP;
    const int ch = tid % CH, r0 = tid / CH;
    const int n0 = ntile * BN + ch * 4;
    const bool vn = n0 < p.Cout;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && vn) bias4 = *reinterpret_cast<const float4*>(p.bias + n0);
    const bool bnb = p.bnb_scale != nullptr;
    float4 bsc = bias4, bsh = bias4, bmu = bias4, bis = bias4;
    if (bnb && vn) {
        bsc = *reinterpret_cast<const float4*>(p.bnb_scale + n0);
        bsh = *reinterpret_cast<const float4*>(p.bnb_shift + n0);
        bmu = *reinterpret_cast<const float4*>(p.bnb_mean + n0);
        bis = *reinterpret_cast<const float4*>(p.bnb_invstd + n0);
    } else if (p.tail.amax_bn && vn) {         // (the two uses exclude each other: the registers are shared)
        bsc = *reinterpret_cast<const float4*>(p.tail.amax_scale + n0);
        bsh = *reinterpret_cast<const float4*>(p.tail.amax_shift + n0);
    }
    const float am2lo = p.tail.amax_relu ? 0.f : -__builtin_inff();
    float am2 = 0.f;                           // max |relu?(written value * scale + shift)| (p.tail.amax_bn)
    // fp16x3: the accumulators hold (A s_a)(W s_w); both scales are powers of two, the product is undone exactly
    const float osc = p.a_bound ? 1.f / (pow2_scale(bound64(p.a_bound)) * pow2_scale(bound64(p.w_bound))) : 1.f;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    float am = 0.f;                            // max |written value| (p.tail.amax)
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
    float4 r1[NP], r2[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int m = rowmap(r0 + RPP * (gi * NP + j));
        const bool ok = vn && m < p.M;
        const size_t o = ok ? (size_t)m * p.Cout + n0 : 0;
        r1[j] = p.res1 ? *reinterpret_cast<const float4*>(p.res1 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        r2[j] = p.res2 ? *reinterpret_cast<const float4*>(p.res2 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int row = r0 + RPP * (gi * NP + j);
        const int m = rowmap(row);
        if (vn && m < p.M) {
            float4 v = *reinterpret_cast<const float4*>(Cs + row * CP + ch * 4);
            v.x *= osc; v.y *= osc; v.z *= osc; v.w *= osc;
            if (bnb) {
                // v = dL/d relu(bn(x)); r1[j] = x: mask by the ReLU, accumulate the BN-backward sums
                const float4 xv = r1[j];
                if (p.bnb_relu) {
                    if (fmaf(xv.x, bsc.x, bsh.x) <= 0.f) v.x = 0.f;
                    if (fmaf(xv.y, bsc.y, bsh.y) <= 0.f) v.y = 0.f;
                    if (fmaf(xv.z, bsc.z, bsh.z) <= 0.f) v.z = 0.f;
                    if (fmaf(xv.w, bsc.w, bsh.w) <= 0.f) v.w = 0.f;
                }
                *reinterpret_cast<float4*>(p.y + (size_t)m * p.Cout + n0) = v;
                s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
                s2.x = fmaf(v.x, (xv.x - bmu.x) * bis.x, s2.x); s2.y = fmaf(v.y, (xv.y - bmu.y) * bis.y, s2.y);
                s2.z = fmaf(v.z, (xv.z - bmu.z) * bis.z, s2.z); s2.w = fmaf(v.w, (xv.w - bmu.w) * bis.w, s2.w);
                am = fmaxf(fmaxf(am, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));      // max |dz| (p.tail.amax)
                continue;
            }
            v.x += bias4.x + r1[j].x + r2[j].x; v.y += bias4.y + r1[j].y + r2[j].y;
            v.z += bias4.z + r1[j].z + r2[j].z; v.w += bias4.w + r1[j].w + r2[j].w;
            *reinterpret_cast<float4*>(p.y + (size_t)m * p.Cout + n0) = v;
            am = fmaxf(fmaxf(am, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
            if (p.tail.amax_bn)
                am2 = fmaxf(fmaxf(am2, fabsf(fmaxf(fmaf(v.x, bsc.x, bsh.x), am2lo))),
                            fmaxf(fabsf(fmaxf(fmaf(v.y, bsc.y, bsh.y), am2lo)),
                                  fmaxf(fabsf(fmaxf(fmaf(v.z, bsc.z, bsh.z), am2lo)), fabsf(fmaxf(fmaf(v.w, bsc.w, bsh.w), am2lo)))));
            s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
            s2.x = fmaf(v.x, v.x, s2.x); s2.y = fmaf(v.y, v.y, s2.y);
            s2.z = fmaf(v.z, v.z, s2.z); s2.w = fmaf(v.w, v.w, s2.w);
        }
    }
    }
    if (p.tail.amax) amax_commit(am, p.tail.amax);
    if (p.tail.amax_bn) amax_commit(am2, p.tail.amax_bn, 1);
    if (p.stats) {
        __syncthreads();                       // every thread has read its part of Cs
        float* red = smem;                     // [RPP][BN][2]
        float* mine = red + ((size_t)r0 * BN + ch * 4) * 2;
        mine[0] = s1.x; mine[1] = s2.x; mine[2] = s1.y; mine[3] = s2.y;
        mine[4] = s1.z; mine[5] = s2.z; mine[6] = s1.w; mine[7] = s2.w;
        __syncthreads();
        if (tid < BN) {
            const int n = ntile * BN + tid;
            if (n < p.Cout) {
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int w = 0; w < RPP; ++w) {
                    a0 += red[((size_t)w * BN + tid) * 2 + 0];
                    a1 += red[((size_t)w * BN + tid) * 2 + 1];
                }
                tail_store(p.stats + ((size_t)mtile * 2 + 0) * p.Cout + n, a0);
                tail_store(p.stats + ((size_t)mtile * 2 + 1) * p.Cout + n, a1);
            }
        }
    }
}
