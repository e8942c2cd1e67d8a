// Heat-map distillation: a teacher-student loss on the logits, and its gradient with respect to the student's, in one
// launch.  Rows: head_row.h.  Per student row s and teacher row t of n = H*W logits, temperature T:
//   lq = log_softmax(s / T), lp = log_softmax(t / T), q = exp(lq), p = exp(lp)
//   kind 1 (kl):  L = T^2 sum p (lp - lq)                                       dL/ds = T (q - p)
//   kind 0 (js):  lm = logaddexp(lp, lq) - ln 2,  L = T^2 (sum p (lp - lm) + sum q (lq - lm)) / 2
//   kind 2 (mse): L = T^2 sum (q - p)^2
//   js, mse:      dL/ds_j = T q_j (v_j - sum_i q_i v_i),  v = (lq - lm) / 2 (js), 2 (q - p) (mse)
// Everything is formed from the scaled, shifted logits a = (x - max x) / T and log Z = log sum exp(a): a peaked row's
// probabilities underflow in fp32, its log-probabilities a - log Z do not, and there is no eps.  A term whose p or q has
// underflowed contributes 0.
// HBM-bound: a workgroup holds ONE teacher row (a and p: 32 floats per thread for H*W <= 4096) and walks the student rows
// that pair with it, r = t, t + teacher_rows, ...: the teacher's maximum, exponentials and sum are formed once, and every
// map is read from HBM once — 2 + 1/S map passes for rows = S teacher_rows (student in, gradient out, teacher in).
// Longer rows are re-read (served by L2) instead of held.  Every sum is a fixed tree over the workgroup: the result does
// not depend on the launch.
#include "head_row.h"

#define LN2 0.69314718055994530942f

// A row of logits as the softmax of x / T needs it: a_i = (x_i - max x) / T, p_i = exp(a_i) / Z, log Z.
// CACHED: a and p stay in registers.  Otherwise the row is read again and both are formed again, by the same expressions.
template <int VEC, bool CACHED>
struct SoftRow {
    Row<VEC, CACHED> a;
    float pr[16];
    float m, invt, z, invz, logz;
    __device__ __forceinline__ void load(const float* src, int hw, float inv_t, float* red) {
        a.load(src, hw);
        invt = inv_t;
        float mx = -INFINITY;
        a.each([&](int, float v) { mx = fmaxf(mx, v); });
        m = block_max(mx, red);
        float s[1] = {0.f};
        if (CACHED) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                a.v[k] = (a.v[k] - m) * invt;
                pr[k] = fast_exp(a.v[k]);
            }
            a.each_slot([&](int k, int, float) { s[0] += pr[k]; });
        } else {
            a.each([&](int, float v) { s[0] += fast_exp((v - m) * invt); });
        }
        block_sum<1>(s, red);
        z = s[0];
        invz = 1.f / z;
        logz = logf(z);
        if (CACHED) {
#pragma unroll
            for (int k = 0; k < 16; ++k) pr[k] *= invz;
        }
    }
};

// f(slot, i, at, p, as, q) for every element this thread owns of a teacher and a student row of the same length
template <int VEC, bool CACHED, typename F>
__device__ __forceinline__ void each_pair(const SoftRow<VEC, CACHED>& t, const SoftRow<VEC, CACHED>& s, F f) {
    if (CACHED) {
        s.a.each_slot([&](int k, int i, float as) { f(k, i, t.a.v[k], t.pr[k], as, s.pr[k]); });
    } else {
        s.a.each([&](int i, float x) {
            const float as = (x - s.m) * s.invt, at = (t.a.src[i] - t.m) * t.invt;
            f(0, i, at, fast_exp(at) * t.invz, as, fast_exp(as) * s.invz);
        });
    }
}

// js: tp = lp - lm and tq = lq - lm.  With d = |lp - lq|, lm = max(lp, lq) + u, u = log(1 + exp(-d)) - ln 2 in [-ln 2, 0]:
// one exponential and one hardware log2 (v_log_f32: its absolute error, 1e-7, is what the yardstick measures)
__device__ __forceinline__ void js_terms(float lp, float lq, float& tp, float& tq) {
    const float d = fabsf(lp - lq), mx = fmaxf(lp, lq);
    const float u = fmaf(__builtin_amdgcn_logf(1.f + fast_exp(-d)), LN2, -LN2);
    tp = (lp - mx) - u;
    tq = (lq - mx) - u;
}

template <int VEC>
__device__ __forceinline__ void store_slots(float* __restrict__ out, const float (&g)[16], int hw) {
    const int tid = threadIdx.x;
    if (VEC == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = (k * HB + tid) * 4;
            if (i < hw) *reinterpret_cast<float4*>(out + i) = make_float4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = k * HB + tid;
            if (i < hw) out[i] = g[k];
        }
    }
}

// grid: a multiple of teacher_rows that divides rows.  Workgroup b takes the student rows b, b + grid, ... — all of them
// pair with teacher row b % teacher_rows.  g0 NULL: values only (the same instructions up to the stores, so the same
// loss_row bits as the launch with g0 whenever both take the same <VEC, CACHED> variant).
template <int VEC, bool CACHED>
__global__ __launch_bounds__(HB) void distill_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                                                      const float* __restrict__ mask, const float* __restrict__ denom_p,
                                                      float* __restrict__ loss_row, float* __restrict__ g0, long rows,
                                                      long teacher_rows, int hw, float temperature, int kind) {
    __shared__ float red[16];
    const float inv_t = 1.f / temperature, t2 = temperature * temperature;
    const float den = mask ? denom_p[1] : (float)rows;
    SoftRow<VEC, CACHED> t;
    t.load(teacher + (size_t)(blockIdx.x % teacher_rows) * hw, hw, inv_t, red);
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float wm = (mask ? mask[r] : 1.f) / den;
        SoftRow<VEC, CACHED> s;
        s.load(student + (size_t)r * hw, hw, inv_t, red);
        const float f = wm * temperature;
        const bool live = g0 != nullptr && wm != 0.f;      // a row of weight 0: a gradient of exactly 0, whatever its logits
        float* out = g0 ? g0 + (size_t)r * hw : nullptr;
        float gv[16];
        float acc[2] = {0.f, 0.f};
        float val;
        if (kind == 1) {
            // sum p (lp - lq) = sum p ((at - as) + log(Zs / Zt)): one pass, the gradient needs no sum.  The logarithm of the
            // quotient, not the difference of two logarithms: near convergence it is small and so is its rounding
            const float dl = logf(s.z / t.z);
            each_pair(t, s, [&](int k, int i, float at, float p, float as, float q) {
                acc[0] = fmaf(p, (at - as) + dl, acc[0]);
                const float g = live ? f * (q - p) : 0.f;
                if (CACHED) gv[k] = g;
                else if (g0) out[i] = g;
            });
            float s1[1] = {acc[0]};
            block_sum<1>(s1, red);
            val = t2 * s1[0];
        } else {
            // v_i and the two sums: acc[0] completes the value, acc[1] = sum q v
            auto terms = [&](float at, float p, float as, float q, float& v) {
                if (kind == 0) {
                    float tp, tq;
                    js_terms(at - t.logz, as - s.logz, tp, tq);
                    v = 0.5f * tq;
                    return p * tp;                            // sum p tp + sum q tq = sum p tp + 2 sum q v
                }
                const float d = q - p;
                v = 2.f * d;
                return d * d;
            };
            each_pair(t, s, [&](int k, int, float at, float p, float as, float q) {
                float v;
                acc[0] += terms(at, p, as, q, v);
                acc[1] = fmaf(q, v, acc[1]);
                if (CACHED) gv[k] = v;
            });
            block_sum<2>(acc, red);
            val = kind == 0 ? t2 * (0.5f * (acc[0] + 2.f * acc[1])) : t2 * acc[0];
            if (g0) {
                const float c = acc[1];
                each_pair(t, s, [&](int k, int i, float at, float p, float as, float q) {
                    float v;
                    if (CACHED) v = gv[k];
                    else terms(at, p, as, q, v);
                    const float g = live ? f * q * (v - c) : 0.f;
                    if (CACHED) gv[k] = g;
                    else out[i] = g;
                });
            }
        }
        if (CACHED && g0) store_slots<VEC>(out, gv, hw);
        if (threadIdx.x == 0) loss_row[r] = val;
    }
}

static int distill_launch(const char* who, const float* student, const float* teacher, const float* mask,
                          const float* denom2, float* loss_row, float* g_logits, bool grad, int64_t rows,
                          int64_t teacher_rows, int h, int w, float temperature, int kind, void* stream) {
    DSNT_REQUIRE(student && teacher && loss_row && (!grad || g_logits) && (!mask || denom2), DSNT_ERR_ARG,
                 "%s: null tensor", who);
    if (int e = check_rows(who, rows, h, w)) return e;
    DSNT_REQUIRE(teacher_rows > 0 && rows % teacher_rows == 0, DSNT_ERR_SHAPE, "%s: teacher_rows=%lld does not divide rows=%lld",
                 who, (long long)teacher_rows, (long long)rows);
    DSNT_REQUIRE(temperature > 0.f, DSNT_ERR_ARG, "%s: temperature must be positive", who);
    DSNT_REQUIRE(kind >= 0 && kind <= 2, DSNT_ERR_ARG, "%s: unknown kind %d", who, kind);
    // One workgroup per teacher row, walking its student rows, when that alone fills the device; one per student row
    // otherwise (DSNT_OFF=distill_walk: always).  The two grids give the same bits.
    const bool walk = teacher_rows >= 2L * dsnt_device_cus() && !dsnt_kernel_off("distill_walk");
    const int grid = (int)(walk ? teacher_rows : rows);
    // (a g_logits off a 16-byte boundary alone sends dsnt_distill_loss_grad to the one-float variant, whose threads own other
    // elements: its loss_row then differs from dsnt_distill_rows' in the last bits)
    const bool ptr_ok = dsnt_aligned16(student) && dsnt_aligned16(teacher) && (!grad || dsnt_aligned16(g_logits));
    ROW_DISPATCH(distill_kernel, grid, (long)h * w, ptr_ok, student, teacher, mask, denom2, loss_row, g_logits, (long)rows,
                 (long)teacher_rows, h * w, temperature, kind);
    DSNT_CHECK_LAUNCH(who);
}

extern "C" int dsnt_distill_rows(const float* student, const float* teacher, float* loss_row, int64_t rows,
                                 int64_t teacher_rows, int h, int w, float temperature, int kind, void* stream) {
    return distill_launch("dsnt_distill_rows", student, teacher, nullptr, nullptr, loss_row, nullptr, false, rows,
                          teacher_rows, h, w, temperature, kind, stream);
}

extern "C" int dsnt_distill_loss_grad(const float* student, const float* teacher, const float* mask, const float* denom2,
                                      float* loss_row, float* g_logits, int64_t rows, int64_t teacher_rows, int h, int w,
                                      float temperature, int kind, void* stream) {
    return distill_launch("dsnt_distill_loss_grad", student, teacher, mask, denom2, loss_row, g_logits, true, rows,
                          teacher_rows, h, w, temperature, kind, stream);
}
