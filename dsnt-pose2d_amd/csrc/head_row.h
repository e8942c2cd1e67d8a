// What the DSNT head units (head_ops.hip, head_loss.hip, head_fwd.hip) share, and heatmap.hip borrows the host side of.
// HBM-bound: one 256-thread workgroup per (image, joint) row of H*W floats; the row is read from HBM once and kept in
// registers (16 floats per thread for H*W <= 4096, 16-byte loads when H*W % 4 == 0) while wavefront reductions produce
// the softmax denominator, the coordinate moments and the divergence sums.  Longer rows fall back to re-reading the row
// (served by L2).  Meshgrids are never materialised: x_w = (2w - (W-1))/W, y_h = (2h - (H-1))/H.
#pragma once
#include "common.h"
#include "flipmerge.h"
#include <math.h>

#define HB 256   // threads per row

// A row of H*W values read from `SRC`: a plain `const float*` (every kernel but one), or the flip-merged logits of
// dsnt_flip_merge_head (FlipSrc, flipmerge.h), which are formed as they are read.
template <int VEC, bool CACHED, typename SRC = const float*>
struct Row {
    float v[16];
    SRC src;
    int hw;
    __device__ __forceinline__ void load(SRC row, int n) {
        src = row; hw = n;
        if (CACHED) {
            const int tid = threadIdx.x;
            if (VEC == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = (k * HB + tid) * 4;
                    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (i < hw) t = row_load4(row, i);
                    v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = k * HB + tid;
                    v[k] = i < hw ? row[i] : 0.f;
                }
            }
        }
    }
    // f(slot, index, value) for every element this thread owns (CACHED rows only): slot = 0..15 is a compile-time
    // constant after unrolling, so per-element temporaries indexed by it live in registers
    template <typename F>
    __device__ __forceinline__ void each_slot(F f) const {
        const int tid = threadIdx.x;
        if (VEC == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = (k * HB + tid) * 4;
                if (i < hw) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) f(4 * k + e, i + e, v[4 * k + e]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = k * HB + tid;
                if (i < hw) f(k, i, v[k]);
            }
        }
    }
    // f(index, value) for every element this thread owns
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        const int tid = threadIdx.x;
        if (CACHED) {
            if (VEC == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = (k * HB + tid) * 4;
                    if (i < hw) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) f(i + e, v[4 * k + e]);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = k * HB + tid;
                    if (i < hw) f(i, v[k]);
                }
            }
        } else {
            for (int i = tid; i < hw; i += HB) f(i, src[i]);
        }
    }
};

// exp(x) for x <= 0 on the hardware exp2 (v_exp_f32, <= 1 ulp) with a compensated x * log2(e): the product is formed
// as t + r with t = fl(x L), r = fma(x, L, -t) + x L_lo, so the argument error (|x| 2^-24 for a plain multiply: 2e-6
// relative at x = -30) does not reach the result: e^x = 2^t (1 + r ln 2).  ~6 instructions instead of libm's ~25.
__device__ __forceinline__ float fast_exp(float x) {
    const float L = 1.44269502162933349609375f, Ll = 1.92596299112661746e-8f;
    const float t = x * L;
    const float r = fmaf(x, Ll, fmaf(x, L, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.69314718055994530942f, e);
}

struct Grid2 {
    int W, H; float offx, offy;
    __device__ __forceinline__ Grid2(int h, int w) : W(w), H(h), offx((float)(w - 1)), offy((float)(h - 1)) {}
    __device__ __forceinline__ void xy(int i, float& x, float& y) const {
        const int r = i / W, c = i - r * W;
        x = (2.f * c - offx) / (float)W;   // exact closed form of linspace(-(W-1)/W, (W-1)/W, W)
        y = (2.f * r - offy) / (float)H;
    }
};

// ------------------------------------------------------------------ row statistics (definition: flipmerge.h)
// Two sweeps over the values p of a row.  The first runs where the coordinates are made: every thread feeds each p it
// owns, in ascending index, to a StatAcc, and stats_first reduces peak, first index and mass over the workgroup.  The
// second (stats_cov) needs the mean: `each(f)` calls f(i, p) for every element the thread owns, with the same p.
struct RowStats { float peak, mass, mx, my, vxx, vyy, vxy; int index; };
struct StatAcc {
    float best = -INFINITY, mass = 0.f;
    int bi = 0x7fffffff;
    __device__ __forceinline__ void add(int i, float p) {
        mass += p;
        if (p > best) { best = p; bi = i; }            // ascending i per thread: keeps the first maximum
    }
};

__device__ __forceinline__ void stats_first(const StatAcc& a, float* red, RowStats& st) {
    float s[1] = {a.mass};
    block_sum<1>(s, red);
    st.mass = s[0];
    st.peak = a.best; st.index = a.bi;
    block_peak(st.peak, st.index, red);
}

template <typename EACH>
__device__ __forceinline__ void stats_cov(EACH each, const Grid2& g, float* red, RowStats& st) {
    float v[3] = {0.f, 0.f, 0.f};
    const float mx = st.mx, my = st.my;
    each([&](int i, float p) {
        float x, y; g.xy(i, x, y);
        const float dx = x - mx, dy = y - my;
        v[0] = fmaf(dx * dx, p, v[0]); v[1] = fmaf(dy * dy, p, v[1]); v[2] = fmaf(dx * dy, p, v[2]);
    });
    block_sum<3>(v, red);
    st.vxx = v[0]; st.vyy = v[1]; st.vxy = v[2];
}

__device__ __forceinline__ void stats_store(const RowStats& st, float* __restrict__ stats, int* __restrict__ peak_index,
                                            size_t row) {
    float* o = stats + 7 * row;
    o[0] = st.peak; o[1] = st.mass; o[2] = st.mx; o[3] = st.my; o[4] = st.vxx; o[5] = st.vyy; o[6] = st.vxy;
    peak_index[row] = st.index;
}

// the un-normalised Gaussian about (mx, my), k = -1 / (2 sigma^2): make_gauss and the regularisers must agree bit for bit
__device__ __forceinline__ float gauss_e(float x, float y, float mx, float my, float k) {
    return expf(((x - mx) * (x - mx) + (y - my) * (y - my)) * k);
}

// ------------------------------------------------------------------ preact (model.py:24-45)
// the activation of modes 2..4 (abs, relu, sigmoid) before the division by the row's sum, and
__device__ __forceinline__ float preact_act(int mode, float v) {
    return mode == 2 ? fabsf(v) : mode == 3 ? fmaxf(v, 0.f) : 1.f / (1.f + expf(-v));
}
// the normalised row of every mode: sink(i, y_i) for every element this thread owns, in Row::each order
template <typename ROW, typename SINK>
__device__ __forceinline__ void preact_row(const ROW& row, int mode, float thr, float eps, float* red, SINK sink) {
    if (mode <= 1) {
        float m = -INFINITY;
        row.each([&](int, float v) { m = fmaxf(m, v); });
        m = block_max(m, red);
        float s[1] = {0.f};
        row.each([&](int, float v) {
            const float e = expf(v - m);
            s[0] += (mode == 1 && !(v >= thr)) ? 0.f : e;
        });
        block_sum<1>(s, red);
        const float denom = mode == 1 ? s[0] + eps : s[0];
        row.each([&](int i, float v) {
            const float e = (mode == 1 && !(v >= thr)) ? 0.f : expf(v - m);
            sink(i, e / denom);
        });
    } else {
        float s[1] = {0.f};
        row.each([&](int, float v) { s[0] += preact_act(mode, v); });
        block_sum<1>(s, red);
        const float denom = s[0] + eps;
        row.each([&](int i, float v) { sink(i, preact_act(mode, v) / denom); });
    }
}

// ------------------------------------------------------ fused head forward: one HBM read of the logits
// the row's softmax, stored to `out` when STORE, and its coordinate moments c (block-reduced: every thread has them)
// STATS (dsnt_flip_merge_head_stats): the row's statistics in *st as well, every p fed to them where it is formed.
template <int VEC, bool CACHED, bool STORE, bool STATS = false, typename SRC>
__device__ __forceinline__ void head_fwd_row(Row<VEC, CACHED, SRC>& row, float* __restrict__ out, int h, int w,
                                             float* red, float (&c)[2], RowStats* st = nullptr) {
    const int hw = h * w;
    float m = -INFINITY;
    row.each([&](int, float v) { m = fmaxf(m, v); });
    m = block_max(m, red);
    float s[1] = {0.f};
    if (CACHED) {
        // one exponential per element: they replace the logits in the row registers
#pragma unroll
        for (int k = 0; k < 16; ++k) row.v[k] = fast_exp(row.v[k] - m);
        row.each([&](int, float e) { s[0] += e; });
    } else {
        row.each([&](int, float v) { s[0] += expf(v - m); });
    }
    block_sum<1>(s, red);
    const float denom = s[0];
    const Grid2 g(h, w);
    c[0] = 0.f; c[1] = 0.f;
    StatAcc a;
    if (CACHED && VEC == 4 && (w & 3) == 0) {
        // four consecutive pixels of one heat-map row per 16-byte store: one division for the position, the
        // normalisation as a multiplication by 1 / sum (one more rounding than e / sum: <= 1 ulp)
        const float inv = 1.f / denom;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = (k * HB + threadIdx.x) * 4;
            if (i < hw) {
                const int rr = i / w, cc = i - rr * w;
                const float y = (2.f * rr - g.offy) / (float)h;
                float p[4], px = 0.f, ps = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p[e] = row.v[4 * k + e] * inv;
                    const float x = (2.f * (cc + e) - g.offx) / (float)w;
                    px = fmaf(x, p[e], px);
                    ps += p[e];
                    if (STATS) a.add(i + e, p[e]);
                }
                c[0] += px; c[1] = fmaf(y, ps, c[1]);
                if (STORE) *reinterpret_cast<float4*>(out + i) = make_float4(p[0], p[1], p[2], p[3]);
            }
        }
    } else if (CACHED && VEC == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = (k * HB + threadIdx.x) * 4;
            if (i < hw) {
                float p[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p[e] = row.v[4 * k + e] / denom;
                    float x, y; g.xy(i + e, x, y);
                    c[0] = fmaf(x, p[e], c[0]); c[1] = fmaf(y, p[e], c[1]);
                    if (STATS) a.add(i + e, p[e]);
                }
                if (STORE) *reinterpret_cast<float4*>(out + i) = make_float4(p[0], p[1], p[2], p[3]);
            }
        }
    } else {
        row.each([&](int i, float v) {
            const float p = (CACHED ? v : expf(v - m)) / denom;
            if (STORE) out[i] = p;
            float x, y; g.xy(i, x, y);
            c[0] = fmaf(x, p, c[0]); c[1] = fmaf(y, p, c[1]);
            if (STATS) a.add(i, p);
        });
    }
    block_sum<2>(c, red);
    if constexpr (STATS) {
        stats_first(a, red, *st);
        st->mx = c[0]; st->my = c[1];
        // second sweep: p by the expression of the branch that formed it above, so the same bits.  CACHED rows hold their
        // exponentials in registers; longer rows read the logits again and evaluate expf(v - m) again.
        const bool quad = CACHED && VEC == 4 && (w & 3) == 0;
        const float inv = 1.f / denom;
        stats_cov([&](auto f) {
            row.each([&](int i, float v) { f(i, quad ? v * inv : (CACHED ? v : expf(v - m)) / denom); });
        }, g, red, *st);
    }
}

// ------------------------------------------------------------------ host side
// The <VEC, CACHED> variant every launch of a row kernel takes: rows of up to 4096 pixels are held in registers, and
// loaded 16 bytes at a time when their length is a multiple of 4 and every row pointer involved is aligned (`ptr_ok`).
enum RowVariant { ROW_STREAMED, ROW_CACHED, ROW_CACHED_VEC4 };         // <1, false>, <1, true>, <4, true>
static inline RowVariant row_variant(long hw, bool ptr_ok) {
    return hw > 4096 ? ROW_STREAMED : (hw % 4 == 0 && ptr_ok) ? ROW_CACHED_VEC4 : ROW_CACHED;
}
#define ROW_DISPATCH(KERNEL, rows, hw, ptr_ok, ...)                                                                    \
    switch (row_variant(hw, ptr_ok)) {                                                                                 \
        case ROW_CACHED_VEC4: DSNT_LAUNCH((KERNEL<4, true>), dim3(rows), dim3(HB), 0, stream, __VA_ARGS__); break;     \
        case ROW_CACHED: DSNT_LAUNCH((KERNEL<1, true>), dim3(rows), dim3(HB), 0, stream, __VA_ARGS__); break;          \
        case ROW_STREAMED: DSNT_LAUNCH((KERNEL<1, false>), dim3(rows), dim3(HB), 0, stream, __VA_ARGS__); break;       \
    }

static int check_rows(const char* who, int64_t rows, int h, int w) {
    DSNT_REQUIRE(rows > 0 && rows < (1LL << 31), DSNT_ERR_SHAPE, "%s: rows=%lld out of range", who, (long long)rows);
    DSNT_REQUIRE(h > 0 && w > 0 && (long)h * w < (1L << 24), DSNT_ERR_SHAPE, "%s: bad map size %dx%d", who, h, w);
    return DSNT_OK;
}
static inline float gauss_k(float sigma) { return (float)(-0.5 * (1.0 / (double)sigma) * (1.0 / (double)sigma)); }
