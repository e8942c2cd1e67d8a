// The PCKh evaluators (evaluator.py:66, train.py:243-258): the hit test at one threshold and the one-launch histogram
// behind the PCKh curve, both on one fp64 distance expression.
#include "common.h"

// ---------------------------------------------------------------- PCKh hits
// Distance of joint i (of image n) between the back-projected prediction and target, in head lengths: one expression for
// pckh_kernel and pckh_hist_kernel, so that the curve at a threshold holds the very hits of the single-threshold kernel.
__device__ __forceinline__ double pckh_distance(const float* __restrict__ pred, const float* __restrict__ target,
                                                const double* __restrict__ m, const double* __restrict__ b,
                                                const double* __restrict__ head, long i, long n) {
    const double* mm = m + (size_t)n * 4;
    const double* bb = b + (size_t)n * 2;
    const double px = pred[2 * i], py = pred[2 * i + 1], tx = target[2 * i], ty = target[2 * i + 1];
    // row-vector times matrix plus offset (train.py:243-258: bmm(norm, transform_m) + transform_b)
    const double ox = px * mm[0] + py * mm[2] + bb[0], oy = px * mm[1] + py * mm[3] + bb[1];
    const double gx = tx * mm[0] + ty * mm[2] + bb[0], gy = tx * mm[1] + ty * mm[3] + bb[1];
    return sqrt((ox - gx) * (ox - gx) + (oy - gy) * (oy - gy)) / head[n];
}
__global__ void pckh_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                            const double* __restrict__ m, const double* __restrict__ b,
                            const float* __restrict__ mask, const double* __restrict__ head,
                            float thr, float* hits, float* valid, int B, int J) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * J) return;
    const double d = pckh_distance(pred, target, m, b, head, i, i / J);
    const bool v = mask[i] == 1.f;
    valid[i] = v ? 1.f : 0.f;
    hits[i] = (v && d <= (double)thr) ? 1.f : 0.f;
}
extern "C" int dsnt_pckh(const float* pred, const float* target, const double* m, const double* b,
                         const float* mask, const double* head, float threshold, float* hits,
                         float* valid, int B, int J, void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && hits && valid && B > 0 && J > 0,
                 DSNT_ERR_ARG, "dsnt_pckh: bad argument");
    DSNT_LAUNCH(pckh_kernel, dim3((B * J + 255) / 256), dim3(256), 0, (hipStream_t)stream, pred,
                       target, m, b, mask, head, threshold, hits, valid, B, J);
    DSNT_CHECK_LAUNCH("dsnt_pckh");
}

// PCKh curve: a histogram of d per joint with the thresholds as bin edges (include/dsnt_hip.h: dsnt_pckh_hist).  Integer adds
// only, so the table does not depend on the order of arrival.  At most DSNT_PCKH_HIST_MAX_BLOCKS workgroups stride over
// B * J; with use_lds each counts in an LDS copy of the table (u32: a workgroup sees fewer than 2^31 joints) and flushes
// its non-zero cells with one 64-bit atomic each, so the global traffic is bounded by grid x cells whatever the batch.
static_assert(DSNT_PCKH_HIST_MAX_T % 8 == 0, "pckh_hist_kernel reads the edges eight at a time");
struct pckh_thresholds { double t[DSNT_PCKH_HIST_MAX_T]; };
__global__ __launch_bounds__(DSNT_PCKH_HIST_BLOCK)
void pckh_hist_kernel(const float* __restrict__ pred, const float* __restrict__ target, const double* __restrict__ m,
                      const double* __restrict__ b, const float* __restrict__ mask, const double* __restrict__ head,
                      const pckh_thresholds thr, int T, unsigned long long* table, double* dist, int B, int J, int use_lds) {
    __shared__ unsigned cnt[DSNT_PCKH_HIST_LDS_CELLS];
    const int cells = J * (T + 1);
    if (use_lds) {
        for (int c = threadIdx.x; c < cells; c += blockDim.x) cnt[c] = 0u;
        __syncthreads();
    }
    const long total = (long)B * J;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / J;
        const int j = (int)(i - n * J);
        const double d = pckh_distance(pred, target, m, b, head, i, n);
        const bool v = mask[i] == 1.f;
        if (dist) dist[i] = v ? d : (double)NAN;
        if (!v) continue;
        // ascending edges: the thresholds d exceeds are a prefix, and their number is the bin.  The index is uniform, so
        // eight edges are one scalar load of the kernel argument; the host pads the edges with +inf, which only a NaN
        // exceeds (NaN exceeds all: bin T).
        int k = 0;
        for (int q = 0; q < T; q += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) k += (d <= thr.t[q + u]) ? 0 : 1;
        }
        k = min(k, T);
        const int c = j * (T + 1) + k;
        if (use_lds) atomicAdd(cnt + c, 1u);
        else atomicAdd(table + c, 1ull);
    }
    if (use_lds) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += blockDim.x) {
            const unsigned v = cnt[c];
            if (v) atomicAdd(table + c, (unsigned long long)v);
        }
    }
}
extern "C" int dsnt_pckh_hist(const float* pred, const float* target, const double* m, const double* b,
                              const float* mask, const double* head, const double* thresholds, int T,
                              unsigned long long* table, double* dist, int B, int J, void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && thresholds && table && B > 0 && J > 0,
                 DSNT_ERR_ARG, "dsnt_pckh_hist: bad argument");
    DSNT_REQUIRE(T >= 1 && T <= DSNT_PCKH_HIST_MAX_T, DSNT_ERR_ARG, "dsnt_pckh_hist: T=%d outside 1..%d", T,
                 DSNT_PCKH_HIST_MAX_T);
    DSNT_REQUIRE((long)J * (T + 1) <= 0x7fffffffL, DSNT_ERR_ARG, "dsnt_pckh_hist: J * (T + 1) does not fit an int");
    pckh_thresholds thr;
    for (int k = 0; k < DSNT_PCKH_HIST_MAX_T; ++k) thr.t[k] = (double)INFINITY;
    for (int k = 0; k < T; ++k) {
        const double t = thresholds[k];
        DSNT_REQUIRE(t - t == 0.0, DSNT_ERR_ARG, "dsnt_pckh_hist: threshold %d is not finite", k);
        DSNT_REQUIRE(k == 0 || t > thresholds[k - 1], DSNT_ERR_ARG,
                     "dsnt_pckh_hist: thresholds must be strictly ascending (index %d)", k);
        thr.t[k] = t;
    }
    const long total = (long)B * J;
    const long want = (total + DSNT_PCKH_HIST_BLOCK - 1) / DSNT_PCKH_HIST_BLOCK;
    const int grid = (int)(want < DSNT_PCKH_HIST_MAX_BLOCKS ? want : DSNT_PCKH_HIST_MAX_BLOCKS);
    const int use_lds = (long)J * (T + 1) <= DSNT_PCKH_HIST_LDS_CELLS ? 1 : 0;
    DSNT_LAUNCH(pckh_hist_kernel, dim3(grid), dim3(DSNT_PCKH_HIST_BLOCK), 0, (hipStream_t)stream, pred, target, m, b,
                mask, head, thr, T, table, dist, B, J, use_lds);
    DSNT_CHECK_LAUNCH("dsnt_pckh_hist");
}
