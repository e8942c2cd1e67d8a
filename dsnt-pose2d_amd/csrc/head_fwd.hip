// From logits to heat-maps and coordinates: softmax + expectation in one pass (dsnt_head_fwd), the flip-merged head of
// batched evaluation and the statistics of stored heat-maps, each followed by its entry points.  Rows: head_row.h.
#include "head_row.h"

template <int VEC, bool CACHED>
__global__ __launch_bounds__(HB) void head_fwd_kernel(const float* __restrict__ logits, float* __restrict__ hm,
                                                       float* __restrict__ coords, int h, int w) {
    __shared__ float red[16];
    const size_t off = (size_t)blockIdx.x * h * w;
    Row<VEC, CACHED> row;
    row.load(logits + off, h * w);
    float c[2];
    head_fwd_row<VEC, CACHED, true>(row, hm + off, h, w, red, c);
    if (threadIdx.x == 0) { coords[2 * (size_t)blockIdx.x] = c[0]; coords[2 * (size_t)blockIdx.x + 1] = c[1]; }
}

extern "C" int dsnt_head_fwd(const float* logits, float* hm, float* coords, int64_t rows, int h, int w, void* stream) {
    DSNT_REQUIRE(logits && hm && coords, DSNT_ERR_ARG, "dsnt_head_fwd: null tensor");
    if (int e = check_rows("dsnt_head_fwd", rows, h, w)) return e;
    ROW_DISPATCH(head_fwd_kernel, (int)rows, h * w, dsnt_aligned16(logits) && dsnt_aligned16(hm), logits, hm,
                 coords, h, w);
    DSNT_CHECK_LAUNCH("dsnt_head_fwd");
}

// ------------------------------------------------------------------ flip-merged head (inference.py:38-57)
// One workgroup per (sample b, joint j) row of the merged logits (flipmerge.h), read through a FlipSrc: softmax through
// head_fwd_row (dsnt_head_fwd's arithmetic), the other preactivations through preact_row (dsnt_preact_fwd's) with
// dsnt_expect_fwd's expectation in the sink; the same VEC / CACHED variant those launches take on the merged tensor, so
// the coordinates are theirs bit for bit.  Thread 0 back-projects them in fp64.
// With a StatsOut (dsnt_flip_merge_head_stats) the row's statistics (flipmerge.h) come out of the same launch: peak, first
// index and mass from the p the head's own loops form, the covariance from a second sweep that reads no heat-map.
// Softmax: head_fwd_row sweeps the row registers again (CACHED), or reads the logits again and evaluates the
// exponential again (rows of more than 4096 pixels: no registers to hold them, and no LDS size that fits every such
// row).  The other preactivations: preact_row runs a second time on the row it already holds, the same code and so the
// same p, at the price of its two reductions and one more activation per pixel; nothing but the logits is ever read.
// Sums run in the order of dsnt_heatmap_stats on the stored heat-maps, so the two agree bit for bit; the one exception
// is softmax rows whose width is a multiple of 4.  There head_fwd_row sums four pixels at a time (the coordinates'
// order, which the mean must keep) and normalises by a multiplication that the compiler contracts into the sums (the
// mass adds e * (1 / sum) without rounding p first), so mass, mean and the covariance about that mean agree with
// dsnt_heatmap_stats to fp32 rounding, not bit for bit.  Peak and index are exact everywhere.
template <int VEC, bool CACHED, bool STORE, typename... ST>
__global__ __launch_bounds__(HB) void flip_merge_dsnt_kernel(const float* __restrict__ logits, int B, int J, int h,
                                                              int w, FlipPerm perm, int mode, float thr, float eps,
                                                              const double* __restrict__ tm,
                                                              const double* __restrict__ tb, float* __restrict__ hm,
                                                              float* __restrict__ coords, double* __restrict__ img,
                                                              ST... so) {
    constexpr bool STATS = sizeof...(ST) > 0;
    __shared__ float red[16];
    const int row = blockIdx.x, hw = h * w;
    Row<VEC, CACHED, FlipSrc> r;
    r.load(flip_src(logits, B, J, hw, w, perm, row), hw);
    float* out = STORE ? hm + (size_t)row * hw : nullptr;
    float c[2] = {0.f, 0.f};
    RowStats st;
    if (mode == 0) {
        head_fwd_row<VEC, CACHED, STORE, STATS>(r, out, h, w, red, c, &st);
    } else {
        const Grid2 g(h, w);
        StatAcc a;
        preact_row(r, mode, thr, eps, red, [&](int i, float p) {
            if (STORE) out[i] = p;
            float x, y; g.xy(i, x, y);
            c[0] = fmaf(x, p, c[0]); c[1] = fmaf(y, p, c[1]);
            if (STATS) a.add(i, p);
        });
        block_sum<2>(c, red);
        if constexpr (STATS) {
            stats_first(a, red, st);
            st.mx = c[0]; st.my = c[1];
            stats_cov([&](auto f) { preact_row(r, mode, thr, eps, red, f); }, g, red, st);
        }
    }
    if (threadIdx.x == 0) {
        coords[2 * (size_t)row] = c[0];
        coords[2 * (size_t)row + 1] = c[1];
        flip_backproject(c[0], c[1], tm, tb, img, row / J, row);
        if constexpr (STATS) {
            const StatsOut o = only(so...);
            stats_store(st, o.stats, o.peak_index, row);
            stats_cov_image(st.vxx, st.vyy, st.vxy, tm, o.cov_image, row / J, row);
        }
    }
}

// dsnt_flip_merge_head (so == NULL) and dsnt_flip_merge_head_stats: one validation, one dispatch
static int flip_merge_head_impl(const char* who, const float* logits, int64_t B, int J, int h, int w, const int* perm,
                                int strategy, int preact, float threshold, float eps, const double* transform_m,
                                const double* transform_b, float* hm, float* coords, double* img, const StatsOut* so,
                                void* stream) {
    DSNT_REQUIRE(logits && perm && transform_m && transform_b && coords && img, DSNT_ERR_ARG, "%s: null pointer", who);
    DSNT_REQUIRE(!so || (so->stats && so->peak_index && so->cov_image), DSNT_ERR_ARG, "%s: null pointer", who);
    DSNT_REQUIRE(strategy == DSNT_FLIP_DSNT || strategy == DSNT_FLIP_GAUSS, DSNT_ERR_ARG, "%s: unknown strategy %d", who,
                 strategy);
    DSNT_REQUIRE(strategy != DSNT_FLIP_DSNT || (preact >= 0 && preact <= 4), DSNT_ERR_ARG, "%s: unknown preact mode %d",
                 who, preact);
    DSNT_REQUIRE(J > 0 && J <= DSNT_FLIP_MAX_J, DSNT_ERR_SHAPE, "%s: J=%d outside 1..%d", who, J, DSNT_FLIP_MAX_J);
    DSNT_REQUIRE(B > 0 && 2 * B * J < (1LL << 31), DSNT_ERR_SHAPE, "%s: B=%lld out of range", who, (long long)B);
    if (int e = check_rows(who, 2 * B * J, h, w)) return e;
    FlipPerm fp = {};
    unsigned seen = 0;
    for (int j = 0; j < J; ++j) {
        DSNT_REQUIRE(perm[j] >= 0 && perm[j] < J && !(seen >> perm[j] & 1u), DSNT_ERR_ARG,
                     "%s: perm is not a permutation of 0..%d (perm[%d] = %d)", who, J - 1, j, perm[j]);
        seen |= 1u << perm[j];
        fp.p[j] = perm[j];
    }
    if (strategy == DSNT_FLIP_GAUSS) {
        flip_merge_decode_launch(logits, (int)B, J, h, w, fp, transform_m, transform_b, hm, coords, img, so, stream);
        DSNT_CHECK_LAUNCH(who);
    }
    // the variant dsnt_head_fwd / dsnt_preact_fwd + dsnt_expect_fwd pick for the (16-byte aligned) merged tensor
    const RowVariant variant = row_variant(h * w, dsnt_aligned16(logits) && (!hm || dsnt_aligned16(hm)));
    const dim3 grid((unsigned)(B * J));
    hipStream_t st = (hipStream_t)stream;
    const StatsOut o = so ? *so : StatsOut{};
#define FLIP_LAUNCH(V, C, S)                                                                                              \
    do {                                                                                                                  \
        if (so)                                                                                                           \
            DSNT_LAUNCH((flip_merge_dsnt_kernel<V, C, S, StatsOut>), grid, dim3(HB), 0, st, logits, (int)B, J, h, w, fp,  \
                        preact, threshold, eps, transform_m, transform_b, hm, coords, img, o);                            \
        else                                                                                                              \
            DSNT_LAUNCH((flip_merge_dsnt_kernel<V, C, S>), grid, dim3(HB), 0, st, logits, (int)B, J, h, w, fp, preact,    \
                        threshold, eps, transform_m, transform_b, hm, coords, img);                                       \
    } while (0)
    switch (variant) {
        case ROW_CACHED_VEC4: if (hm) FLIP_LAUNCH(4, true, true); else FLIP_LAUNCH(4, true, false); break;
        case ROW_CACHED: if (hm) FLIP_LAUNCH(1, true, true); else FLIP_LAUNCH(1, true, false); break;
        case ROW_STREAMED: if (hm) FLIP_LAUNCH(1, false, true); else FLIP_LAUNCH(1, false, false); break;
    }
#undef FLIP_LAUNCH
    DSNT_CHECK_LAUNCH(who);
}

extern "C" int dsnt_flip_merge_head(const float* logits, int64_t B, int J, int h, int w, const int* perm, int strategy,
                                    int preact, float threshold, float eps, const double* transform_m,
                                    const double* transform_b, float* hm, float* coords, double* img, void* stream) {
    return flip_merge_head_impl("dsnt_flip_merge_head", logits, B, J, h, w, perm, strategy, preact, threshold, eps,
                                transform_m, transform_b, hm, coords, img, nullptr, stream);
}

extern "C" int dsnt_flip_merge_head_stats(const float* logits, int64_t B, int J, int h, int w, const int* perm,
                                          int strategy, int preact, float threshold, float eps,
                                          const double* transform_m, const double* transform_b, float* hm, float* coords,
                                          double* img, float* stats, int* peak_index, double* cov_image, void* stream) {
    const StatsOut so = {stats, peak_index, cov_image};
    return flip_merge_head_impl("dsnt_flip_merge_head_stats", logits, B, J, h, w, perm, strategy, preact, threshold, eps,
                                transform_m, transform_b, hm, coords, img, &so, stream);
}

// dsnt_heatmap_stats: the statistics of a materialised heat-map tensor.  The first sweep is expect_fwd_kernel's (the mean
// is dsnt_expect_fwd's bit for bit) with the mass and the peak beside it; CACHED rows are read from HBM once, longer ones
// are read again for the second sweep.
template <int VEC, bool CACHED>
__global__ __launch_bounds__(HB) void heatmap_stats_kernel(const float* __restrict__ hm, float* __restrict__ stats,
                                                            int* __restrict__ peak_index, int h, int w) {
    __shared__ float red[16];
    const int hw = h * w;
    Row<VEC, CACHED> row;
    row.load(hm + (size_t)blockIdx.x * hw, hw);
    const Grid2 g(h, w);
    StatAcc a;
    float s[2] = {0.f, 0.f};
    row.each([&](int i, float p) {
        float x, y; g.xy(i, x, y);
        s[0] = fmaf(x, p, s[0]); s[1] = fmaf(y, p, s[1]);
        a.add(i, p);
    });
    block_sum<2>(s, red);
    RowStats st;
    stats_first(a, red, st);
    st.mx = s[0]; st.my = s[1];
    stats_cov([&](auto f) { row.each(f); }, g, red, st);
    if (threadIdx.x == 0) stats_store(st, stats, peak_index, blockIdx.x);
}

extern "C" int dsnt_heatmap_stats(const float* hm, int64_t rows, int h, int w, float* stats, int* peak_index,
                                  void* stream) {
    DSNT_REQUIRE(hm && stats && peak_index, DSNT_ERR_ARG, "dsnt_heatmap_stats: null tensor");
    if (int e = check_rows("dsnt_heatmap_stats", rows, h, w)) return e;
    ROW_DISPATCH(heatmap_stats_kernel, (int)rows, h * w, dsnt_aligned16(hm), hm, stats, peak_index, h, w);
    DSNT_CHECK_LAUNCH("dsnt_heatmap_stats");
}
