// What bn.hip and resample.hip share: the thread mapping of the 128-row tile kernels and the element-wise op + BatchNorm statistics
// kernel that both launch (tile_op_stats_kernel: OP 0 / 1 from resample.hip, OP 2 from bn.hip).
#pragma once
#include "common.h"
#include "bn_pro.h"

#define TILE_ROWS 128
// Thread mapping of the tile kernels (tile_reduce_kernel in bn.hip, tile_op_stats_kernel below), host side, shared so that
// their sums stay bit-identical to each other: a workgroup covers `cgs` float4 column groups x (256 / cgs) row lanes of one 128-row tile.  Large tensors: all columns in one
// workgroup (up to 256 groups per pass).  Small ones (fewer than 256 tiles — the low-resolution hourglass levels, where
// a 4..64-workgroup launch is pure latency): 16 column groups per workgroup, the rest of the columns on gridDim.y, so a
// thread walks 8 rows instead of 32 and the launch has 4x (C = 256) the workgroups.
static inline int tile_cgs(long tiles, int C4) { return tiles < 256 && C4 > 16 && C4 % 16 == 0 ? 16 : (C4 < 256 ? C4 : 256); }
static inline unsigned tile_grid_y(long tiles, int C4) { const int c = tile_cgs(tiles, C4); return c == 16 && C4 > 16 ? C4 / 16 : 1; }

struct TileOpP {
    const float* a; const float* b; float* y; unsigned char* idx; float* partial;
    int N, Ho, Wo, C, cgs;
    OutBoundsP tail;
    const float* bn_scale; const float* bn_shift; int bn_relu;
};
// (OP 0 / 1 / 2: resample.hip and bn.hip describe the family at their entry points.  bx, by, gy: blockIdx.x, blockIdx.y, gridDim.y;
// red: 256 * 8 floats of LDS.  Still a device function under its kernel: written into the kernel, OP 2 needs two more VGPRs.)
template <int OP>
__device__ __forceinline__ void tile_op_stats_body(const TileOpP& q, const int bx, const int by, const int gy, float* red) {
    const float* __restrict__ a = q.a; const float* __restrict__ b = q.b; float* __restrict__ y = q.y;
    unsigned char* __restrict__ idx = q.idx; float* partial = q.partial;
    const int N = q.N, Ho = q.Ho, Wo = q.Wo, C = q.C, cgs = q.cgs;
    const OutBoundsP tail = q.tail;
    const float* __restrict__ bn_scale = q.bn_scale; const float* __restrict__ bn_shift = q.bn_shift; const int bn_relu = q.bn_relu;
    const int tid = threadIdx.x;
    const int C4 = C >> 2;
    const int rpar = 256 / cgs;
    const int cg_l = tid % cgs, rl = tid / cgs;
    const bool active = rl < rpar;
    const long M = (long)N * Ho * Wo;
    const long row0 = (long)bx * TILE_ROWS;
    const long row1 = row0 + TILE_ROWS < M ? row0 + TILE_ROWS : M;
    float am = 0.f;                                  // max |written value| (tail.amax: fp16x3 bound of a raw consumer)
    float am2 = 0.f;                                 // max |relu?(written value * scale + shift)| (tail.amax_bn)
    const float am2lo = tail.amax_relu ? 0.f : -__builtin_inff();
    for (int cg0 = by * cgs; cg0 < C4; cg0 += cgs * gy) {
        const int cg = cg0 + cg_l;
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
        if (active && cg < C4) {
            // batches of UB rows: every load of the batch is issued before the first use (a workgroup of a small level is
            // pure latency), rows are then consumed in the same order as one by one — the sums stay bit-identical to
            // tile_reduce_kernel<0>.  (Built WITHOUT the SLP vectoriser: see build.py.)
#ifndef DSNT_TILE_UB
#define DSNT_TILE_UB 1        // measured: 4 is no faster once small tensors use the 16-lane mapping
#endif
            constexpr int UB = DSNT_TILE_UB;
            float4 bs = make_float4(0.f, 0.f, 0.f, 0.f), bh = bs;
            if (tail.amax_bn) {
                bs = reinterpret_cast<const float4*>(tail.amax_scale)[cg];
                bh = reinterpret_cast<const float4*>(tail.amax_shift)[cg];
            }
            for (long rb = row0 + rl; rb < row1; rb += (long)UB * rpar) {
                float4 in[UB][OP == 0 ? 4 : 2];
                float4 osc = make_float4(0.f, 0.f, 0.f, 0.f), osh = osc;
                if (OP == 2) {
                    osc = reinterpret_cast<const float4*>(bn_scale)[cg];
                    osh = reinterpret_cast<const float4*>(bn_shift)[cg];
                }
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const long r = rb + (long)u * rpar < row1 ? rb + (long)u * rpar : row1 - 1;     // clamped: never used
                    const int ow = (int)(r % Wo);
                    const long t = r / Wo;
                    const int oh = (int)(t % Ho), n = (int)(t / Ho);
                    if (OP == 0) {
                        const int W = Wo * 2;
                        const float4* base = reinterpret_cast<const float4*>(a) + (((long)n * (Ho * 2) + 2 * oh) * W + 2 * ow) * C4 + cg;
                        in[u][0] = base[0]; in[u][1] = base[C4];
                        in[u][OP == 0 ? 2 : 0] = base[(long)W * C4]; in[u][OP == 0 ? 3 : 1] = base[(long)W * C4 + C4];
                    } else if (OP == 1) {
                        in[u][0] = reinterpret_cast<const float4*>(a)[r * C4 + cg];
                        in[u][1] = reinterpret_cast<const float4*>(b)[(((long)n * (Ho >> 1) + (oh >> 1)) * (Wo >> 1) + (ow >> 1)) * C4 + cg];
                    } else {
                        in[u][0] = reinterpret_cast<const float4*>(a)[r * C4 + cg];
                    }
                }
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const long r = rb + (long)u * rpar;
                    if (r >= row1) break;
                    float4 v;
                    if (OP == 0) {
                        const float4 v1 = in[u][1], v2 = in[u][OP == 0 ? 2 : 0], v3 = in[u][OP == 0 ? 3 : 1];
                        v = in[u][0];
                        uchar4 k = make_uchar4(0, 0, 0, 0);
#define POOL_STEP(V, P)                                  \
                        if (V.x > v.x || V.x != V.x) { v.x = V.x; k.x = P; } \
                        if (V.y > v.y || V.y != V.y) { v.y = V.y; k.y = P; } \
                        if (V.z > v.z || V.z != V.z) { v.z = V.z; k.z = P; } \
                        if (V.w > v.w || V.w != V.w) { v.w = V.w; k.w = P; }
                        POOL_STEP(v1, 1) POOL_STEP(v2, 2) POOL_STEP(v3, 3)
#undef POOL_STEP
                        reinterpret_cast<uchar4*>(idx)[r * C4 + cg] = k;
                    } else if (OP == 1) {
                        const float4 uu = in[u][0], l = in[u][1];
                        v = make_float4(uu.x + l.x, uu.y + l.y, uu.z + l.z, uu.w + l.w);
                    } else {
                        const float4 xv = in[u][0];
                        v = make_float4(fmaf(xv.x, osc.x, osh.x), fmaf(xv.y, osc.y, osh.y), fmaf(xv.z, osc.z, osh.z),
                                        fmaf(xv.w, osc.w, osh.w));
                        if (bn_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    }
                    reinterpret_cast<float4*>(y)[r * C4 + cg] = v;
                    am = fmaxf(fmaxf(am, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
                    if (tail.amax_bn)
                        am2 = fmaxf(fmaxf(am2, fabsf(fmaxf(fmaf(v.x, bs.x, bh.x), am2lo))),
                                    fmaxf(fabsf(fmaxf(fmaf(v.y, bs.y, bh.y), am2lo)),
                                          fmaxf(fabsf(fmaxf(fmaf(v.z, bs.z, bh.z), am2lo)), fabsf(fmaxf(fmaf(v.w, bs.w, bh.w), am2lo)))));
                    s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
                    s2.x = fmaf(v.x, v.x, s2.x); s2.y = fmaf(v.y, v.y, s2.y);
                    s2.z = fmaf(v.z, v.z, s2.z); s2.w = fmaf(v.w, v.w, s2.w);
                }
            }
        }
        if (!partial) continue;                       // eval mode: only the operand bound is wanted (uniform)
        __syncthreads();
        float* mine = red + tid * 8;
        mine[0] = s1.x; mine[1] = s1.y; mine[2] = s1.z; mine[3] = s1.w;
        mine[4] = s2.x; mine[5] = s2.y; mine[6] = s2.z; mine[7] = s2.w;
        __syncthreads();
        if (tid < cgs && cg0 + tid < C4) {
            float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < rpar; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += red[(j * cgs + tid) * 8 + e];
            float* p0 = partial + ((size_t)bx * 2 + 0) * C + (size_t)(cg0 + tid) * 4;
            float* p1 = partial + ((size_t)bx * 2 + 1) * C + (size_t)(cg0 + tid) * 4;
            *reinterpret_cast<float4*>(p0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            *reinterpret_cast<float4*>(p1) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        }
    }
    if (tail.amax) amax_commit(am, tail.amax, 0);
    if (tail.amax_bn) amax_commit(am2, tail.amax_bn, 1);
}

template <int OP>
__global__ __launch_bounds__(256) void tile_op_stats_kernel(TileOpP q) {
    __shared__ __attribute__((aligned(16))) float red[256 * 8];
    tile_op_stats_body<OP>(q, blockIdx.x, blockIdx.y, gridDim.y, red);
}
