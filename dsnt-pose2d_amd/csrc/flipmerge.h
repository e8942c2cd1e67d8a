// dsnt_flip_merge_head (head.hip: entry point and the dsnt strategy; heatmap.hip: the gauss strategy): the flip-merged
// logits of a paired batch, computed where they are read instead of being materialised.
//
// logits [2B][J][h][w], rows B..2B-1 the mirrored inputs.  The merged row of (sample b, joint j) is
//   m[y][x] = (L[b][j][y][x] + L[B + b][perm[j]][y][w - 1 - x]) / 2
// in fp32, the reference's `(hm1 + hm2) / 2` of inference.py:41-46 (the division by 2 is exact: the same value as
// ATen's).  A FlipSrc stands in for the `const float*` a row is read from: Row<> (head.hip) and the arg-max decode
// (heatmap.hip) take either.
#pragma once
#include "common.h"

#define DSNT_FLIP_MAX_J 32

struct FlipPerm { int p[DSNT_FLIP_MAX_J]; };     // passed by value in the kernel arguments

struct FlipSrc {
    const float* a;      // L[b][j]
    const float* m;      // L[B + b][perm[j]]
    int w;
    __device__ __forceinline__ float operator[](int i) const {
        const int r = i / w, c = i - r * w;
        return (a[i] + m[r * w + (w - 1 - c)]) / 2.f;
    }
};

// four consecutive values from index i (i % 4 == 0, 16-byte aligned rows): the plain row, or the merged one
__device__ __forceinline__ float4 row_load4(const float* p, int i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ float4 row_load4(const FlipSrc& s, int i) {
    const float4 x = *reinterpret_cast<const float4*>(s.a + i);
    const int r = i / s.w, c = i - r * s.w;
    if ((s.w & 3) == 0) {      // the four mirrored pixels are one aligned float4 of the same row, reversed
        const float4 y = *reinterpret_cast<const float4*>(s.m + r * s.w + (s.w - 4 - c));
        return make_float4((x.x + y.w) / 2.f, (x.y + y.z) / 2.f, (x.z + y.y) / 2.f, (x.w + y.x) / 2.f);
    }
    return make_float4((x.x + s.m[r * s.w + (s.w - 1 - c)]) / 2.f, s[i + 1], s[i + 2], s[i + 3]);
}

__device__ __forceinline__ FlipSrc flip_src(const float* logits, int B, int J, int hw, int w, const FlipPerm& perm,
                                            int row) {
    const int b = row / J, j = row - b * J;
    return FlipSrc{logits + (size_t)row * hw, logits + ((size_t)(B + b) * J + perm.p[j]) * hw, w};
}

// inference.py:54-57: baddbmm(transform_b, coords.double(), transform_m) for one joint: img = t + c . M in fp64
__device__ __forceinline__ void flip_backproject(float cx, float cy, const double* __restrict__ tm,
                                                 const double* __restrict__ tb, double* __restrict__ img, int B_idx,
                                                 int row) {
    const double* M = tm + 4 * (size_t)B_idx;
    const double* t = tb + 2 * (size_t)B_idx;
    const double x = cx, y = cy;
    img[2 * (size_t)row] = t[0] + fma(y, M[2], x * M[0]);
    img[2 * (size_t)row + 1] = t[1] + fma(y, M[3], x * M[1]);
}

// the gauss strategy's launch (heatmap.hip); the entry point validates first
int flip_merge_decode_launch(const float* logits, int B, int J, int h, int w, const FlipPerm& perm,
                             const double* tm, const double* tb, float* hm, float* coords, double* img, void* stream);
