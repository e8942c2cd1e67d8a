// Heat-map matching ("gauss" output strategy, the hourglass builder's default): target rendering, the
// mean-squared-error loss against it and its gradient, and arg-max decoding of predicted heat-maps.
// Replaces /root/reference/src/dsnt/util.py:70-198 (draw_gaussian / encode_heatmaps / get_preds /
// decode_heatmaps: CPU loops over B x J maps with a D2H copy per step) and the loss of
// /root/reference/src/dsnt/model.py:147-156, 247-258.  HBM-bound, one 256-thread workgroup per
// (image, joint) row of H*W floats; the 7x7 target bump is evaluated in-register, never materialised
// for the loss.
#include "head_row.h"   // HB, check_rows, gauss_k; common.h and flipmerge.h

// The reference's coordinate arithmetic is a chain of separately rounded fp32 tensor ops (add_, mul_, add_);
// hipcc contracts a*b+c into one FMA by default (and HIP's __fmul_rn / __fadd_rn are plain operators), which
// moves results by an ulp and can move a rounded pixel.  This file is compiled with -ffp-contract=off
// (build.py; HIP's default -ffp-contract=fast ignores `#pragma clang fp contract`).

// Centre of the target bump of a row: util.py:133-146 — pixel = (c + 1) * (W/2) - 0.5 in fp32, three separately
// rounded operations (no FMA contraction), then Python round() = round-half-even; draw_gaussian (:70-126) with
// clip_size 7 (radius 3.5) skips bumps whose centre is more than 3.5 px outside the map.
struct Bump {
    int x, y, x0, x1, y0, y1;   // centre and clipped window [x0, x1) x [y0, y1); empty window when skipped
};
__device__ __forceinline__ Bump bump_of(const float* __restrict__ target, long row, int h, int w) {
    // w / 2 and h / 2 are exact in fp32 (integers or halves)
    const float cx = target[2 * row], cy = target[2 * row + 1];
    const float px = __fadd_rn(__fmul_rn(__fadd_rn(cx, 1.f), (float)(w / 2.0)), -0.5f);
    const float py = __fadd_rn(__fmul_rn(__fadd_rn(cy, 1.f), (float)(h / 2.0)), -0.5f);
    Bump b;
    b.x = (int)rintf(px); b.y = (int)rintf(py);
    const float radius = 3.5f;
    const bool skip = !(px == px) || !(py == py) || b.x <= -radius || b.y <= -radius ||
                      b.x >= (w - 1) + radius || b.y >= (h - 1) + radius;
    b.x0 = max(0, b.x - 3); b.x1 = min(w, b.x + 4);
    b.y0 = max(0, b.y - 3); b.y1 = min(h, b.y + 4);
    if (skip) { b.x0 = b.x1 = 0; b.y0 = b.y1 = 0; }
    return b;
}
__device__ __forceinline__ float bump_at(const Bump& b, int r, int c, float k) {
    if (c < b.x0 || c >= b.x1 || r < b.y0 || r >= b.y1) return 0.f;
    const float dx = (float)(c - b.x), dy = (float)(r - b.y);
    return expf(__fmul_rn(__fadd_rn(dx * dx, dy * dy), k));        // small integers: dx*dx, dy*dy exact
}

__global__ __launch_bounds__(HB) void encode_heatmaps_kernel(const float* __restrict__ target, float* __restrict__ out,
                                                              int h, int w, float k) {
    const long row = blockIdx.x;
    const Bump b = bump_of(target, row, h, w);
    float* o = out + (size_t)row * h * w;
    for (int i = threadIdx.x; i < h * w; i += HB) {
        const int r = i / w, c = i - r * w;
        o[i] = bump_at(b, r, c, k);
    }
}

// per_row[row] = sum_i (hm[i] - g[i])^2
__global__ __launch_bounds__(HB) void heatmap_mse_fwd_kernel(const float* __restrict__ hm, const float* __restrict__ target,
                                                              float* __restrict__ per_row, int h, int w, float k) {
    __shared__ float red[8];
    const long row = blockIdx.x;
    const Bump b = bump_of(target, row, h, w);
    const float* x = hm + (size_t)row * h * w;
    float s[1] = {0.f};
    for (int i = threadIdx.x; i < h * w; i += HB) {
        const int r = i / w, c = i - r * w;
        const float d = x[i] - bump_at(b, r, c, k);
        s[0] = fmaf(d, d, s[0]);
    }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) per_row[row] = s[0];
}

// dhm[i] = gscale * coef * (hm[i] - g[i]),  coef = 2 / numel
__global__ __launch_bounds__(HB) void heatmap_mse_bwd_kernel(const float* __restrict__ hm, const float* __restrict__ target,
                                                              const float* __restrict__ gscale, float* __restrict__ dhm,
                                                              int h, int w, float k, float coef) {
    const long row = blockIdx.x;
    const Bump b = bump_of(target, row, h, w);
    const float* x = hm + (size_t)row * h * w;
    float* o = dhm + (size_t)row * h * w;
    const float gs = gscale[0] * coef;
    for (int i = threadIdx.x; i < h * w; i += HB) {
        const int r = i / w, c = i - r * w;
        o[i] = gs * (x[i] - bump_at(b, r, c, k));
    }
}

// torch.max's order on (value, index) pairs: does (ov, oi) come before (v, i)?  NaN above every number, NaN beside NaN
// and equal numbers by the lower index.  Without a NaN this is `ov > v || (ov == v && oi < i)`.
__device__ __forceinline__ bool argmax_before(float ov, int oi, float v, int i) {
    const bool on = ov != ov, vn = v != v;
    if (on || vn) return on && (!vn || oi < i);
    return ov > v || (ov == v && oi < i);
}

// util.py:150-198: first arg-max pixel, (0, 0) when the maximum is not positive, +-0.25 px towards the larger
// neighbour for interior pixels, then pixel -> normalised coordinates ((p + 0.5) * (2/size) - 1, fp32 steps).
// The arg-max is torch.max's: a NaN is the maximum and the first NaN's index the arg-max, so a row that holds a NaN
// decodes to pixel (0, 0) (`peak` NaN is not positive) with `index` at its first NaN.
// One row read from `x` (a `const float*`, or the flip-merged logits of dsnt_flip_merge_head: FlipSrc); thread 0 returns
// true with the coordinates in (cx, cy), the maximum in `peak` and its first index in `index`.  `seen(v)` is called with
// every value a thread reads (the statistics of dsnt_flip_merge_head_stats take the row's sum there).
template <typename SRC, typename F>
__device__ __forceinline__ bool decode_row(const SRC& x, int h, int w, int use_neighbours, float sx, float sy, float& cx,
                                           float& cy, float& peak, int& index, F seen) {
    __shared__ float rv[4];
    __shared__ int ri[4];
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < h * w; i += HB) {
        const float v = x[i];
        seen(v);
        // ascending i per thread: keeps the first maximum, and the first NaN once one is met
        if (v > best || (v != v && best == best)) { best = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (argmax_before(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { rv[wave] = best; ri[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < HB / 64; ++wv)
            if (argmax_before(rv[wv], ri[wv], best, bi)) { best = rv[wv]; bi = ri[wv]; }
        if (bi == 0x7fffffff) bi = 0;                    // all -inf rows
        peak = best; index = bi;
        float px = (float)(bi % w), py = (float)(bi / h);          // `idx / height` as the reference (util.py:161)
        if (!(best > 0.f)) { px = 0.f; py = 0.f; }
        if (use_neighbours) {
            const int xi = (int)px, yi = (int)py;
            if (xi > 0 && xi < w - 1 && yi > 0 && yi < h - 1) {
                const float dxn = x[yi * w + xi + 1] - x[yi * w + xi - 1];
                const float dyn = x[(yi + 1) * w + xi] - x[(yi - 1) * w + xi];
                px += 0.25f * (float)((dxn > 0.f) - (dxn < 0.f));
                py += 0.25f * (float)((dyn > 0.f) - (dyn < 0.f));
            }
        }
        // sx = float(2 / w), sy = float(2 / h) rounded on the host exactly like the reference's Python scalars
        cx = __fadd_rn(__fmul_rn(__fadd_rn(px, 0.5f), sx), -1.f);
        cy = __fadd_rn(__fmul_rn(__fadd_rn(py, 0.5f), sy), -1.f);
        return true;
    }
    return false;
}
template <typename SRC>
__device__ __forceinline__ bool decode_row(const SRC& x, int h, int w, int use_neighbours, float sx, float sy, float& cx,
                                           float& cy) {
    float peak;
    int index;
    return decode_row(x, h, w, use_neighbours, sx, sy, cx, cy, peak, index, [](float) {});
}

__global__ __launch_bounds__(HB) void decode_heatmaps_kernel(const float* __restrict__ hm, float* __restrict__ coords,
                                                              int h, int w, int use_neighbours, float sx, float sy) {
    const long row = blockIdx.x;
    float cx, cy;
    if (decode_row(hm + (size_t)row * h * w, h, w, use_neighbours, sx, sy, cx, cy)) {
        coords[2 * row + 0] = cx;
        coords[2 * row + 1] = cy;
    }
}

// dsnt_flip_merge_head, gauss strategy (model.py:268-269 on the merged heat-maps of inference.py:38-48): the merged row
// is stored when hm != NULL, then decoded as dsnt_decode_heatmaps does (use_neighbours = 1) and back-projected.
// With a StatsOut (dsnt_flip_merge_head_stats; flipmerge.h): peak and first index are the decode's own arg-max, the mass
// is summed in the decode's read of the row (each thread's values in ascending index, then block_sum: not the order of
// dsnt_heatmap_stats on the stored map), and mean, covariance and cov_image are NaN: the map is no distribution.
template <bool STORE, typename... ST>
__global__ __launch_bounds__(HB) void flip_merge_decode_kernel(const float* __restrict__ logits, int B, int J, int h,
                                                                int w, FlipPerm perm, float sx, float sy,
                                                                const double* __restrict__ tm,
                                                                const double* __restrict__ tb, float* __restrict__ hm,
                                                                float* __restrict__ coords, double* __restrict__ img,
                                                                ST... so) {
    constexpr bool STATS = sizeof...(ST) > 0;
    const int row = blockIdx.x, hw = h * w;
    const FlipSrc x = flip_src(logits, B, J, hw, w, perm, row);
    if (STORE) {
        float* o = hm + (size_t)row * hw;
        for (int i = threadIdx.x; i < hw; i += HB) o[i] = x[i];
    }
    float cx, cy;
    if constexpr (STATS) {
        __shared__ float red[4];
        float peak = 0.f, mass[1] = {0.f};
        int index = 0;
        const bool lead = decode_row(x, h, w, 1, sx, sy, cx, cy, peak, index, [&](float v) { mass[0] += v; });
        block_sum<1>(mass, red);
        if (lead) {
            coords[2 * (size_t)row] = cx;
            coords[2 * (size_t)row + 1] = cy;
            flip_backproject(cx, cy, tm, tb, img, row / J, row);
            const StatsOut o = only(so...);
            const float nan = __int_as_float(0x7fc00000);
            float* s = o.stats + 7 * (size_t)row;
            s[0] = peak; s[1] = mass[0];
            for (int k = 2; k < 7; ++k) s[k] = nan;
            o.peak_index[row] = index;
            for (int k = 0; k < 4; ++k) o.cov_image[4 * (size_t)row + k] = (double)nan;
        }
    } else {
        if (decode_row(x, h, w, 1, sx, sy, cx, cy)) {
            coords[2 * (size_t)row] = cx;
            coords[2 * (size_t)row + 1] = cy;
            flip_backproject(cx, cy, tm, tb, img, row / J, row);
        }
    }
}

int flip_merge_decode_launch(const float* logits, int B, int J, int h, int w, const FlipPerm& perm, const double* tm,
                             const double* tb, float* hm, float* coords, double* img, const StatsOut* so, void* stream) {
    const float sx = (float)(2.0 / (double)w), sy = (float)(2.0 / (double)h);
    const dim3 grid((unsigned)(B * J));
    hipStream_t st = (hipStream_t)stream;
    if (so) {
        const StatsOut o = *so;
        if (hm)
            DSNT_LAUNCH((flip_merge_decode_kernel<true, StatsOut>), grid, dim3(HB), 0, st, logits, B, J, h, w, perm, sx, sy,
                        tm, tb, hm, coords, img, o);
        else
            DSNT_LAUNCH((flip_merge_decode_kernel<false, StatsOut>), grid, dim3(HB), 0, st, logits, B, J, h, w, perm, sx,
                        sy, tm, tb, hm, coords, img, o);
        return DSNT_OK;
    }
    if (hm)
        DSNT_LAUNCH(flip_merge_decode_kernel<true>, dim3((unsigned)(B * J)), dim3(HB), 0, (hipStream_t)stream, logits, B,
                    J, h, w, perm, sx, sy, tm, tb, hm, coords, img);
    else
        DSNT_LAUNCH(flip_merge_decode_kernel<false>, dim3((unsigned)(B * J)), dim3(HB), 0, (hipStream_t)stream, logits,
                    B, J, h, w, perm, sx, sy, tm, tb, hm, coords, img);
    return DSNT_OK;
}

static int check_rows_hm(const char* who, int64_t rows, int h, int w, float sigma) {
    if (int e = check_rows(who, rows, h, w)) return e;
    DSNT_REQUIRE(sigma > 0.f, DSNT_ERR_ARG, "%s: sigma must be positive", who);
    return DSNT_OK;
}

extern "C" int dsnt_encode_heatmaps(const float* target, float* out, int64_t rows, int h, int w, float sigma,
                                    void* stream) {
    DSNT_REQUIRE(target && out, DSNT_ERR_ARG, "dsnt_encode_heatmaps: null tensor");
    if (int e = check_rows_hm("dsnt_encode_heatmaps", rows, h, w, sigma)) return e;
    DSNT_LAUNCH(encode_heatmaps_kernel, dim3((unsigned)rows), dim3(HB), 0, (hipStream_t)stream, target, out,
                       h, w, gauss_k(sigma));
    DSNT_CHECK_LAUNCH("dsnt_encode_heatmaps");
}

extern "C" int dsnt_heatmap_mse_fwd(const float* hm, const float* target, float* per_row, int64_t rows, int h,
                                    int w, float sigma, void* stream) {
    DSNT_REQUIRE(hm && target && per_row, DSNT_ERR_ARG, "dsnt_heatmap_mse_fwd: null tensor");
    if (int e = check_rows_hm("dsnt_heatmap_mse_fwd", rows, h, w, sigma)) return e;
    DSNT_LAUNCH(heatmap_mse_fwd_kernel, dim3((unsigned)rows), dim3(HB), 0, (hipStream_t)stream, hm, target,
                       per_row, h, w, gauss_k(sigma));
    DSNT_CHECK_LAUNCH("dsnt_heatmap_mse_fwd");
}

extern "C" int dsnt_heatmap_mse_bwd(const float* hm, const float* target, const float* gscale, float* dhm,
                                    int64_t rows, int h, int w, float sigma, void* stream) {
    DSNT_REQUIRE(hm && target && gscale && dhm, DSNT_ERR_ARG, "dsnt_heatmap_mse_bwd: null tensor");
    if (int e = check_rows_hm("dsnt_heatmap_mse_bwd", rows, h, w, sigma)) return e;
    const float coef = (float)(2.0 / ((double)rows * h * w));
    DSNT_LAUNCH(heatmap_mse_bwd_kernel, dim3((unsigned)rows), dim3(HB), 0, (hipStream_t)stream, hm, target,
                       gscale, dhm, h, w, gauss_k(sigma), coef);
    DSNT_CHECK_LAUNCH("dsnt_heatmap_mse_bwd");
}

extern "C" int dsnt_decode_heatmaps(const float* hm, float* coords, int64_t rows, int h, int w, int use_neighbours,
                                    void* stream) {
    DSNT_REQUIRE(hm && coords, DSNT_ERR_ARG, "dsnt_decode_heatmaps: null tensor");
    if (int e = check_rows_hm("dsnt_decode_heatmaps", rows, h, w, 1.f)) return e;
    DSNT_LAUNCH(decode_heatmaps_kernel, dim3((unsigned)rows), dim3(HB), 0, (hipStream_t)stream, hm, coords, h,
                       w, use_neighbours, (float)(2.0 / (double)w), (float)(2.0 / (double)h));
    DSNT_CHECK_LAUNCH("dsnt_decode_heatmaps");
}
