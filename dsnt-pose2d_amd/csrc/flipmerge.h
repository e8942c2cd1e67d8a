// dsnt_flip_merge_head (head_fwd.hip: entry point and the dsnt strategy; heatmap.hip: the gauss strategy): the flip-merged
// logits of a paired batch, computed where they are read instead of being materialised.
//
// logits [2B][J][h][w], rows B..2B-1 the mirrored inputs.  The merged row of (sample b, joint j) is
//   m[y][x] = (L[b][j][y][x] + L[B + b][perm[j]][y][w - 1 - x]) / 2
// in fp32, the reference's `(hm1 + hm2) / 2` of inference.py:41-46 (the division by 2 is exact: the same value as
// ATen's).  A FlipSrc stands in for the `const float*` a row is read from: Row<> (head_row.h) and the arg-max decode
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

// ---- per-joint statistics of a heat-map row (dsnt_heatmap_stats, dsnt_flip_merge_head_stats)
// For one row (sample b, joint j) with the post-activation map p[y][x], h x w, and the DSNT grid X = (2x + 1)/w - 1,
// Y = (2y + 1)/h - 1 (Grid2, head_row.h):
//   peak, peak_index   max p and the first index i = y w + x that holds it (decode_row's rule); NaN is never the peak
//   mass               sum p (1 for softmax; not for the other preactivations at eps, nor for gauss)
//   mean = (mx, my)    (sum X p, sum Y p): for the dsnt strategy the coordinates, bit for bit
//   cov                vxx = sum (X - mx)^2 p, vyy = sum (Y - my)^2 p, vxy = sum (X - mx)(Y - my) p, by a second sweep
//                      over the row once the mean is known (as reg_context does for `var`), never E[X^2] - mx^2
//   cov_image          f64 [2][2] = M^T S M, S = [[vxx, vxy], [vxy, vyy]], M = transform_m[b]: with img = t + c . M on row
//                      vectors (flip_backproject) the covariance of the joint in original-image pixels^2
// stats f32 [rows][7] = peak, mass, mx, my, vxx, vyy, vxy; peak_index int32 [rows]; cov_image f64 [rows][4].
// For the gauss strategy peak, peak_index and mass describe the merged map as it is and the rest is NaN.
// Thread 0 of the row's workgroup writes everything with plain stores.
//
// The fused kernels take the outputs as an optional trailing parameter pack (`ST... so`, empty or one StatsOut), so the
// instantiations without it keep exactly the signature, and the code, they had.
struct StatsOut {
    float* stats;
    int* peak_index;
    double* cov_image;
};
template <typename T>
__device__ __forceinline__ const T& only(const T& t) { return t; }

// Block-wide (max, first index holding it) from each thread's (best, bi) over ascending indices of its own; bi =
// 0x7fffffff where a thread saw nothing above -inf.  Indices are < 2^24 (check_rows), exact as floats, so the first index
// is a block_max of the negated candidates.  A row with nothing above -inf gives index 0.  Every thread gets the result.
__device__ __forceinline__ void block_peak(float& best, int& bi, float* red) {
    const float m = block_max(best, red);
    const float cand = (best == m && bi != 0x7fffffff) ? (float)bi : 16777216.f;
    const float first = -block_max(-cand, red);
    best = m;
    bi = first < 16777216.f ? (int)first : 0;
}

// cov_image = M^T (S M) in fp64, the products in this order (tests/stats_ref.py follows it)
__device__ __forceinline__ void stats_cov_image(float vxx, float vyy, float vxy, const double* __restrict__ tm,
                                                double* __restrict__ cov_image, int B_idx, int row) {
    const double* M = tm + 4 * (size_t)B_idx;
    const double a = vxx, d = vyy, c = vxy;
    const double t00 = a * M[0] + c * M[2], t01 = a * M[1] + c * M[3];      // S M
    const double t10 = c * M[0] + d * M[2], t11 = c * M[1] + d * M[3];
    double* o = cov_image + 4 * (size_t)row;
    o[0] = M[0] * t00 + M[2] * t10;
    o[1] = M[0] * t01 + M[2] * t11;
    o[2] = M[1] * t00 + M[3] * t10;
    o[3] = M[1] * t01 + M[3] * t11;
}

// the gauss strategy's launch (heatmap.hip); the entry point validates first.  `so`: the statistics' outputs, or NULL.
int flip_merge_decode_launch(const float* logits, int B, int J, int h, int w, const FlipPerm& perm,
                             const double* tm, const double* tb, float* hm, float* coords, double* img,
                             const StatsOut* so, void* stream);
