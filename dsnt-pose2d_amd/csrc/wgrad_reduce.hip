// Slab reduction of the weight gradients: dw[Cout][K] = sum over the slabs ws[slab][Cout][K] that any of the weight-gradient
// kernels (wgrad_gemm.hip, wgrad3.hip, wgrad1.hip, stem4.hip) wrote, and the bias gradient from the [slab][Cout] partials behind
// them; in the launch of the convolution itself (wgrad_reduce_launch, from conv_wgrad.hip) or deferred, many convolutions in
// one launch (dsnt_wgrad_reduce_all).  Fixed summation order: deterministic, no atomics.
#include "wgrad.h"

// 32 float4 columns x 8 slab lanes per block, 8 loads in flight per thread.
// RC float4 columns x SL = 256 / RC slab lanes per 256-thread block: a block reads RC * 16 contiguous bytes of every slab (WRED_RC: A/B)
#ifndef WRED_RC
#define WRED_RC 32
#endif
#ifndef WRED_U
#define WRED_U 8        /* independent 16-byte loads in flight per thread */
#endif
__device__ __forceinline__ void wgrad_reduce_body(const float* __restrict__ ws, float* __restrict__ dw,
                                                  float* __restrict__ dbias, int splits, int CK, int Cout,
                                                  int accumulate, int block) {
    constexpr int RC = WRED_RC, SL = 256 / RC;
    __shared__ float4 red[256];
    const int total4 = CK / 4;
    const int col = threadIdx.x % RC, sl = threadIdx.x / RC;
    const int i = block * RC + col;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < total4) {
        int s = sl;
        for (; s + (WRED_U - 1) * SL < splits; s += WRED_U * SL) {
            float4 v[WRED_U];
#pragma unroll
            for (int u = 0; u < WRED_U; ++u)
                v[u] = *reinterpret_cast<const float4*>(ws + (size_t)(s + SL * u) * CK + (size_t)i * 4);
#pragma unroll
            for (int u = 0; u < WRED_U; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
        }
        for (; s < splits; s += SL) {
            const float4 v = *reinterpret_cast<const float4*>(ws + (size_t)s * CK + (size_t)i * 4);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    } else if (dbias && i - total4 < (Cout + 3) / 4) {
        // bias partials live behind the slabs: [splits][Cout]
        const int n0 = (i - total4) * 4;
        const float* b = ws + (size_t)splits * CK;
        for (int s = sl; s < splits; s += SL) {
            const float* q = b + (size_t)s * Cout + n0;
            a.x += q[0]; if (n0 + 1 < Cout) a.y += q[1]; if (n0 + 2 < Cout) a.z += q[2]; if (n0 + 3 < Cout) a.w += q[3];
        }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (sl == 0) {
        for (int j = 1; j < SL; ++j) {
            const float4 v = red[j * RC + col];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        if (i < total4) {
            float4* o = reinterpret_cast<float4*>(dw) + i;
            if (accumulate) { const float4 c = *o; a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w; }
            *o = a;
        } else if (dbias && i - total4 < (Cout + 3) / 4) {
            const int n0 = (i - total4) * 4;
            const float v4[4] = {a.x, a.y, a.z, a.w};
            for (int e = 0; e < 4 && n0 + e < Cout; ++e)
                dbias[n0 + e] = accumulate ? dbias[n0 + e] + v4[e] : v4[e];
        }
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                            float* __restrict__ dbias, int splits, int CK, int Cout,
                                                            int accumulate) {
    wgrad_reduce_body(ws, dw, dbias, splits, CK, Cout, accumulate, blockIdx.x);
}

void wgrad_reduce_launch(const float* ws, float* dw, float* dbias, int slabs, int CK, int Cout, int accumulate,
                         hipStream_t st) {
    const int total = CK / 4 + (Cout + 3) / 4;
    DSNT_LAUNCH(wgrad_reduce_kernel, dim3((total + WRED_RC - 1) / WRED_RC), dim3(256), 0, st, ws, dw, dbias, slabs, CK, Cout,
                accumulate);
}

// Deferred slab reduction of many convolutions in one launch: blockIdx.y = table row
// {ws, dw, dbias (0 = none), splits, Cout*K, Cout, accumulate}, blockIdx.x = 64-column block of that row.
__global__ __launch_bounds__(256) void wgrad_reduce_all_kernel(const long long* __restrict__ table) {
    const long long* t = table + (size_t)blockIdx.y * 7;
    const int CK = (int)t[4], Cout = (int)t[5];
    const int total = CK / 4 + (Cout + 3) / 4;
    if ((int)blockIdx.x * WRED_RC >= total) return;
    wgrad_reduce_body(reinterpret_cast<const float*>(t[0]), reinterpret_cast<float*>(t[1]),
                      reinterpret_cast<float*>(t[2]), (int)t[3], CK, Cout, (int)t[6], blockIdx.x);
}

extern "C" int dsnt_wgrad_reduce_all(const int64_t* table, int rows, int max_blocks, void* stream) {
    DSNT_REQUIRE(table && rows > 0 && rows <= 65535 && max_blocks > 0, DSNT_ERR_ARG, "dsnt_wgrad_reduce_all: bad argument");
    // (max_blocks counts 64-column blocks: the interface's unit)
    DSNT_LAUNCH(wgrad_reduce_all_kernel, dim3((max_blocks * 64 + WRED_RC - 1) / WRED_RC, rows), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)table);
    DSNT_CHECK_LAUNCH("dsnt_wgrad_reduce_all");
}
