// The PCKh evaluators (evaluator.py:66, train.py:243-258): the hit test at one threshold, the one-launch histogram
// behind the PCKh curve and the misprediction field of bin/investigate.py, all on one fp64 distance expression.
#include "common.h"
#include "philox.h"
#include "pckh_dist.h"

// ---------------------------------------------------------------- PCKh hits
// (pckh_distance and its two halves, pckh_project and pckh_between: pckh_dist.h)
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

// The ascending edges of `who` as a kernel takes them in its argument: the n of `host`, finite and strictly ascending, then
// +inf to the end of `out`.  `what` names one of them in the messages.  0 or the error code.
template <int N>
static int ascending_arg(const char* who, const char* what, const double* host, int n, double (&out)[N]) {
    for (int k = 0; k < N; ++k) out[k] = (double)INFINITY;
    for (int k = 0; k < n; ++k) {
        DSNT_REQUIRE(host[k] - host[k] == 0.0, DSNT_ERR_ARG, "%s: %s %d is not finite", who, what, k);
        DSNT_REQUIRE(k == 0 || host[k] > host[k - 1], DSNT_ERR_ARG, "%s: %ss must be strictly ascending (index %d)", who,
                     what, k);
        out[k] = host[k];
    }
    return DSNT_OK;
}

// PCKh curve: a histogram of d per joint with the thresholds as bin edges (include/dsnt_hip.h: dsnt_pckh_hist), and score
// against distance (dsnt_score_hist): the same with a second index, the row of the joint's score among the score edges,
// so table[j][r][k] summed over r is the curve's table bit for bit.  Integer adds only, so the table does not depend on
// the order of arrival.  At most DSNT_PCKH_HIST_MAX_BLOCKS workgroups stride over B * J; with use_lds each counts in an
// LDS copy of the table (u32: a workgroup sees fewer than 2^31 joints) and flushes its non-zero cells with one 64-bit
// atomic each, so the global traffic is bounded by grid x cells whatever the batch.
static_assert(DSNT_PCKH_HIST_MAX_T % 8 == 0, "pckh_column reads the edges eight at a time");
struct pckh_thresholds { double t[DSNT_PCKH_HIST_MAX_T]; };
// Bin of a distance.  Ascending edges: the thresholds d exceeds are a prefix, and their number is the bin.  The index is
// uniform, so eight edges are one scalar load of the kernel argument; the host pads the edges with +inf, which only a NaN
// exceeds (NaN exceeds all: bin T).
__device__ __forceinline__ int pckh_column(const pckh_thresholds& thr, double d, int T) {
    int k = 0;
    for (int q = 0; q < T; q += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) k += (d <= thr.t[q + u]) ? 0 : 1;
    }
    return min(k, T);
}
static_assert(DSNT_SCORE_HIST_MAX_S % 8 == 0, "score_row reads the edges eight at a time");
static_assert(DSNT_SCORE_HIST_LDS_CELLS * sizeof(unsigned) <= 64 * 1024, "the LDS table is a static allocation");
struct score_edges { double e[DSNT_SCORE_HIST_MAX_S]; };
// Row of a score: the number of edges that are <= the score (ascending edges: those are a prefix), S + 1 for a NaN.  The
// host pads the edges with +inf, which only a score of +inf reaches: capped at S.  The index is uniform, so eight edges
// are one scalar load of the kernel argument, as in pckh_column.
__device__ __forceinline__ int score_row(const score_edges& edges, float score, int S) {
    const double s = (double)score;
    int r = 0;
    for (int q = 0; q < S; q += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r += (edges.e[q + u] <= s) ? 1 : 0;
    }
    return s != s ? S + 1 : min(r, S);
}
// The rows of a joint in the table, as the kernel's argument: one (the curve; nothing travels with the launch), or the
// S + 2 score rows.
struct one_row {
    static constexpr bool scored = false;
    __host__ __device__ int rows() const { return 1; }
    __device__ int row(long) const { return 0; }
};
struct score_rows {
    static constexpr bool scored = true;
    const float* __restrict__ score;
    score_edges edges;
    int S;
    __host__ __device__ int rows() const { return S + 2; }
    __device__ int row(long i) const { return score_row(edges, score[i], S); }
};
// The LDS copy is u32 [J][rows][T + 1], LDS_CELLS at the most (32 KiB for the scores).  Only the curve has `dist`, which
// takes NaN where the mask is not 1; with scores a joint that is masked out is skipped before its distance.  `by` comes
// last and the curve reads the mask after the distance: its instantiation is then instruction for instruction the
// kernel it had to itself, with the same argument layout.
template <int LDS_CELLS, typename Rows>
__global__ __launch_bounds__(DSNT_PCKH_HIST_BLOCK)
void joint_table_kernel(const float* __restrict__ pred, const float* __restrict__ target, const double* __restrict__ m,
                        const double* __restrict__ b, const float* __restrict__ mask, const double* __restrict__ head,
                        const pckh_thresholds thr, int T, unsigned long long* table, double* dist, int B, int J,
                        int use_lds, const Rows by) {
    __shared__ unsigned cnt[LDS_CELLS];
    const int cells = J * by.rows() * (T + 1);
    if (use_lds) {
        for (int c = threadIdx.x; c < cells; c += blockDim.x) cnt[c] = 0u;
        __syncthreads();
    }
    const long total = (long)B * J;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        if (Rows::scored && !(mask[i] == 1.f)) continue;
        const long n = i / J;
        const int j = (int)(i - n * J);
        const double d = pckh_distance(pred, target, m, b, head, i, n);
        const bool v = Rows::scored || mask[i] == 1.f;
        if (!Rows::scored && dist) dist[i] = v ? d : (double)NAN;
        if (!v) continue;
        const int c = (j * by.rows() + by.row(i)) * (T + 1) + pckh_column(thr, d, T);
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
// Both entry points from here on: the table fits an int index (`cells` is how the message writes its size), the thresholds,
// one workgroup per DSNT_PCKH_HIST_BLOCK joints up to DSNT_PCKH_HIST_MAX_BLOCKS, and the LDS copy if the table fits it.
template <int LDS_CELLS, typename Rows>
static int joint_table_launch(const char* who, const char* cells, const float* pred, const float* target, const double* m,
                              const double* b, const float* mask, const double* head, const Rows& by,
                              const double* thresholds, int T, unsigned long long* table, double* dist, int B, int J,
                              void* stream) {
    const long n_cells = (long)J * by.rows() * (T + 1);
    DSNT_REQUIRE(n_cells <= 0x7fffffffL, DSNT_ERR_ARG, "%s: %s does not fit an int", who, cells);
    pckh_thresholds thr;
    if (const int rc = ascending_arg(who, "threshold", thresholds, T, thr.t)) return rc;
    const long want = ((long)B * J + DSNT_PCKH_HIST_BLOCK - 1) / DSNT_PCKH_HIST_BLOCK;
    const int grid = (int)(want < DSNT_PCKH_HIST_MAX_BLOCKS ? want : DSNT_PCKH_HIST_MAX_BLOCKS);
    const int use_lds = n_cells <= LDS_CELLS ? 1 : 0;
    const auto kernel = joint_table_kernel<LDS_CELLS, Rows>;
    DSNT_LAUNCH(kernel, dim3(grid), dim3(DSNT_PCKH_HIST_BLOCK), 0, (hipStream_t)stream, pred, target, m, b, mask, head,
                thr, T, table, dist, B, J, use_lds, by);
    DSNT_CHECK_LAUNCH(who);
}
extern "C" int dsnt_pckh_hist(const float* pred, const float* target, const double* m, const double* b,
                              const float* mask, const double* head, const double* thresholds, int T,
                              unsigned long long* table, double* dist, int B, int J, void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && thresholds && table && B > 0 && J > 0,
                 DSNT_ERR_ARG, "dsnt_pckh_hist: bad argument");
    DSNT_REQUIRE(T >= 1 && T <= DSNT_PCKH_HIST_MAX_T, DSNT_ERR_ARG, "dsnt_pckh_hist: T=%d outside 1..%d", T,
                 DSNT_PCKH_HIST_MAX_T);
    return joint_table_launch<DSNT_PCKH_HIST_LDS_CELLS>("dsnt_pckh_hist", "J * (T + 1)", pred, target, m, b, mask, head,
                                                        one_row{}, thresholds, T, table, dist, B, J, stream);
}
extern "C" int dsnt_score_hist(const float* pred, const float* target, const double* m, const double* b,
                               const float* mask, const double* head, const float* score, const double* score_edges_host,
                               int S, const double* thresholds, int T, unsigned long long* table, int B, int J,
                               void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && score && score_edges_host && thresholds && table && B > 0 &&
                 J > 0, DSNT_ERR_ARG, "dsnt_score_hist: bad argument");
    DSNT_REQUIRE(T >= 1 && T <= DSNT_PCKH_HIST_MAX_T, DSNT_ERR_ARG, "dsnt_score_hist: T=%d outside 1..%d", T,
                 DSNT_PCKH_HIST_MAX_T);
    DSNT_REQUIRE(S >= 1 && S <= DSNT_SCORE_HIST_MAX_S, DSNT_ERR_ARG, "dsnt_score_hist: S=%d outside 1..%d", S,
                 DSNT_SCORE_HIST_MAX_S);
    score_rows by{score, {}, S};
    if (const int rc = ascending_arg("dsnt_score_hist", "score edge", score_edges_host, S, by.edges.e)) return rc;
    return joint_table_launch<DSNT_SCORE_HIST_LDS_CELLS>("dsnt_score_hist", "J * (S + 2) * (T + 1)", pred, target, m, b,
                                                         mask, head, by, thresholds, T, table, nullptr, B, J, stream);
}

// Poisson bootstrap over examples (include/dsnt_hip.h: dsnt_pckh_boot): R + 1 copies of the curve's table, copy 0 with
// weight 1 and copy r with the weight w(id, r) of the example, a function of the example's id, the replicate and the seed
// alone.  Integer adds only, so the table does not depend on the order of arrival, nor on how the examples are batched.
static_assert(DSNT_PCKH_BOOT_LDS_CELLS * sizeof(unsigned) <= 64 * 1024, "the LDS table is a static allocation");
static_assert(DSNT_PCKH_BOOT_CHUNK >= 1 && DSNT_PCKH_BOOT_SPAN >= 1, "a workgroup owns at least one copy and one joint");
static_assert(DSNT_PCKH_HIST_MAX_T < 255, "a column fits a byte, 255 marks a joint that does not count");
static_assert(12ull * DSNT_PCKH_BOOT_MAX_B <= 0xffffffffull && 12ull * (DSNT_PCKH_BOOT_MAX_B + 1ull) > 0xffffffffull,
              "a u32 cell holds 12 from every example");
// Weight of a 32-bit uniform: the number of c_k it reaches, Poisson(1) by inverse CDF.
__device__ __forceinline__ unsigned boot_weight(uint32_t u) {
    constexpr uint32_t cdf[12] = DSNT_PCKH_BOOT_CDF;
    unsigned w = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) w += u >= cdf[k] ? 1u : 0u;
    return w;
}
// Workgroup (x, y): the chunks x, x + gridDim.x, ... of `chunk` copies each, and for each of them the spans y,
// y + gridDim.y, ... of DSNT_PCKH_BOOT_SPAN joints of the flat [B * J].  Per span: the column of every joint once, a byte
// in LDS (255: mask != 1); then copy 0, one thread per joint; then the replicates, one thread per (example, Philox call):
// the call's four words are the weights of the replicates 4q + 1 .. 4q + 4, of which those inside the chunk add the weight
// to the cell of each of the example's joints inside the span.  A chunk begins at copy chunk * x, so its first and last
// Philox call may be shared with a neighbour: both compute it, each uses its own words.
__global__ __launch_bounds__(DSNT_PCKH_BOOT_BLOCK)
void pckh_boot_kernel(const float* __restrict__ pred, const float* __restrict__ target, const double* __restrict__ m,
                      const double* __restrict__ b, const float* __restrict__ mask, const double* __restrict__ head,
                      const int64_t* __restrict__ ids, const pckh_thresholds thr, int T, uint64_t seed, int R,
                      unsigned long long* table, int B, int J, int use_lds, int chunk) {
    __shared__ unsigned cnt[DSNT_PCKH_BOOT_LDS_CELLS];
    __shared__ unsigned char col[DSNT_PCKH_BOOT_SPAN];
    constexpr int SPAN = DSNT_PCKH_BOOT_SPAN;
    const int tid = threadIdx.x, per_copy = J * (T + 1);
    const long total = (long)B * J;
    const long spans = (total + SPAN - 1) / SPAN;
    for (long s0 = (long)blockIdx.x * chunk; s0 <= R; s0 += (long)gridDim.x * chunk) {
        const int s1 = (int)(s0 + chunk <= R ? s0 + chunk : (long)R + 1);         // copies [s0, s1)
        const int cells = use_lds ? (s1 - (int)s0) * per_copy : 0;                // of the LDS table
        // the Philox calls whose replicates 4q + 1 .. 4q + 4 meet [max(s0, 1), s1): none if the chunk is copy 0 alone
        const int q0 = ((int)(s0 > 1 ? s0 : 1) - 1) >> 2;
        const int nq = s1 > 1 ? ((s1 - 2) >> 2) - q0 + 1 : 0;
        unsigned long long* out = table + (size_t)s0 * per_copy;
        if (use_lds) {
            for (int c = tid; c < cells; c += blockDim.x) cnt[c] = 0u;
        }
        for (long span = blockIdx.y; span < spans; span += gridDim.y) {
            const long i0 = span * SPAN;
            const int len = (int)(total - i0 < SPAN ? total - i0 : SPAN);
            __syncthreads();                                   // the zeroes above, and the last span's readers of col
            for (int t = tid; t < len; t += blockDim.x) {
                const long i = i0 + t;
                const double d = pckh_distance(pred, target, m, b, head, i, i / J);
                col[t] = mask[i] == 1.f ? (unsigned char)pckh_column(thr, d, T) : (unsigned char)255;
            }
            __syncthreads();
            if (s0 == 0) {
                for (int t = tid; t < len; t += blockDim.x) {
                    const int k = col[t];
                    if (k == 255) continue;
                    const int c = (int)((i0 + t) % J) * (T + 1) + k;
                    if (use_lds) atomicAdd(cnt + c, 1u);
                    else atomicAdd(out + c, 1ull);
                }
            }
            const long n0 = i0 / J;
            const int units = (int)((i0 + len - 1) / J - n0 + 1) * nq;         // at most SPAN examples x (CHUNK + 2) / 4 + 1
            for (int u = tid; u < units; u += blockDim.x) {
                const long n = n0 + u / nq;
                const int q = q0 + u % nq;
                const uint64_t id = (uint64_t)ids[n];
                uint32_t word[4];
                Philox::gen(word, seed, ((uint64_t)(uint32_t)q << 32) | (id >> 32), (uint32_t)id, DSNT_PCKH_BOOT_DOMAIN);
                // the joints of example n inside the span, as offsets into col
                const long lo = n * J > i0 ? n * J : i0, hi = (n + 1) * J < i0 + len ? (n + 1) * J : i0 + len;
                const int j0 = (int)(lo - n * J), t0 = (int)(lo - i0), nj = (int)(hi - lo);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int s = 4 * q + w + 1;
                    const unsigned weight = boot_weight(word[w]);
                    if (s < s0 || s >= s1 || weight == 0u) continue;
                    const int base = (s - (int)s0) * per_copy + j0 * (T + 1);
                    for (int step = 0, t = u % nj; step < nj; ++step, t = t + 1 < nj ? t + 1 : 0) {   // (lanes start apart: banks)
                        const int k = col[t0 + t];
                        if (k == 255) continue;
                        const int c = base + t * (T + 1) + k;
                        if (use_lds) atomicAdd(cnt + c, weight);
                        else atomicAdd(out + c, (unsigned long long)weight);
                    }
                }
            }
        }
        if (use_lds) {
            __syncthreads();
            for (int c = tid; c < cells; c += blockDim.x) {
                const unsigned v = cnt[c];
                if (v) atomicAdd(out + c, (unsigned long long)v);
            }
            __syncthreads();                                   // before the next chunk zeroes the cells
        }
    }
}
extern "C" int dsnt_pckh_boot(const float* pred, const float* target, const double* m, const double* b,
                              const float* mask, const double* head, const int64_t* ids, const double* thresholds, int T,
                              uint64_t seed, int R, unsigned long long* table, int B, int J, void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && ids && thresholds && table && B > 0 && J > 0 && R > 0,
                 DSNT_ERR_ARG, "dsnt_pckh_boot: bad argument");
    DSNT_REQUIRE(T >= 1 && T <= DSNT_PCKH_HIST_MAX_T, DSNT_ERR_ARG, "dsnt_pckh_boot: T=%d outside 1..%d", T,
                 DSNT_PCKH_HIST_MAX_T);
    DSNT_REQUIRE(B <= DSNT_PCKH_BOOT_MAX_B, DSNT_ERR_ARG, "dsnt_pckh_boot: B=%d above %d", B, DSNT_PCKH_BOOT_MAX_B);
    const long per_copy = (long)J * (T + 1);
    DSNT_REQUIRE(per_copy <= 0x7fffffffL && ((long)R + 1) * per_copy <= 0x7fffffffL, DSNT_ERR_ARG,
                 "dsnt_pckh_boot: (R + 1) * J * (T + 1) does not fit an int");
    pckh_thresholds thr;
    if (const int rc = ascending_arg("dsnt_pckh_boot", "threshold", thresholds, T, thr.t)) return rc;
    const int use_lds = per_copy <= DSNT_PCKH_BOOT_LDS_CELLS ? 1 : 0;
    const long fit = use_lds ? DSNT_PCKH_BOOT_LDS_CELLS / per_copy : DSNT_PCKH_BOOT_CHUNK;
    const int chunk = (int)(fit < DSNT_PCKH_BOOT_CHUNK ? fit : DSNT_PCKH_BOOT_CHUNK);
    const long chunks = ((long)R + chunk) / chunk;             // ceil((R + 1) / chunk)
    const long spans = ((long)B * J + DSNT_PCKH_BOOT_SPAN - 1) / DSNT_PCKH_BOOT_SPAN;
    const dim3 grid((unsigned)(chunks < DSNT_PCKH_BOOT_MAX_CHUNK_BLOCKS ? chunks : DSNT_PCKH_BOOT_MAX_CHUNK_BLOCKS),
                    (unsigned)(spans < DSNT_PCKH_BOOT_MAX_SPAN_BLOCKS ? spans : DSNT_PCKH_BOOT_MAX_SPAN_BLOCKS));
    DSNT_LAUNCH(pckh_boot_kernel, grid, dim3(DSNT_PCKH_BOOT_BLOCK), 0, (hipStream_t)stream, pred, target, m, b, mask,
                head, ids, thr, T, seed, R, table, B, J, use_lds, chunk);
    DSNT_CHECK_LAUNCH("dsnt_pckh_boot");
}

// out[i] = values[joint of i][row of score[i]] (include/dsnt_hip.h: dsnt_score_lookup): the calibration table applied to a
// batch of scores.  Plain stores over a grid stride.
__global__ __launch_bounds__(DSNT_SCORE_LOOKUP_BLOCK)
void score_lookup_kernel(const float* __restrict__ score, const score_edges edges, int S, const float* __restrict__ values,
                         int per_joint, float* __restrict__ out, long n, int J) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int j = per_joint ? (int)(i % J) : 0;
        out[i] = values[j * (S + 2) + score_row(edges, score[i], S)];
    }
}
extern "C" int dsnt_score_lookup(const float* score, const double* score_edges_host, int S, const float* values,
                                 int per_joint, float* out, int64_t n, int J, void* stream) {
    DSNT_REQUIRE(score && score_edges_host && values && out && n > 0 && J > 0 && (per_joint == 0 || per_joint == 1),
                 DSNT_ERR_ARG, "dsnt_score_lookup: bad argument");
    DSNT_REQUIRE(S >= 1 && S <= DSNT_SCORE_HIST_MAX_S, DSNT_ERR_ARG, "dsnt_score_lookup: S=%d outside 1..%d", S,
                 DSNT_SCORE_HIST_MAX_S);
    score_edges edges;
    if (const int rc = ascending_arg("dsnt_score_lookup", "score edge", score_edges_host, S, edges.e)) return rc;
    DSNT_REQUIRE((long)J * (S + 2) <= 0x7fffffffL, DSNT_ERR_ARG, "dsnt_score_lookup: J * (S + 2) does not fit an int");
    const long want = ((long)n + DSNT_SCORE_LOOKUP_BLOCK - 1) / DSNT_SCORE_LOOKUP_BLOCK;
    const int grid = (int)(want < DSNT_SCORE_LOOKUP_MAX_BLOCKS ? want : DSNT_SCORE_LOOKUP_MAX_BLOCKS);
    DSNT_LAUNCH(score_lookup_kernel, dim3(grid), dim3(DSNT_SCORE_LOOKUP_BLOCK), 0, (hipStream_t)stream, score, edges, S,
                values, per_joint, out, (long)n, J);
    DSNT_CHECK_LAUNCH("dsnt_score_lookup");
}

// Misprediction field (bin/investigate.py:62-99; include/dsnt_hip.h: dsnt_error_field): per joint, a bins x bins grid over
// the target's location holding how many joints there were, how many missed, and the summed offset of the misses.  The
// sums are fp64 adds, whose result depends on their order, so there are no atomics: workgroup j owns joint j, and lane l
// owns the cells l, l + BLOCK, ... of that joint in all five planes.  The samples are walked in chunks of BLOCK: lane i
// writes the record of sample n0 + i to LDS, then every wave walks the records in ascending n and each lane takes those
// of its own cells, which is the sequential loop over n bit for bit, however the set is cut into calls.
static_assert(DSNT_ERROR_FIELD_BLOCK % 64 == 0 && DSNT_ERROR_FIELD_BLOCK >= 64, "whole waves");
constexpr int EF_CELLS = DSNT_ERROR_FIELD_MAX_BINS * DSNT_ERROR_FIELD_MAX_BINS;
constexpr int EF_OWN = (EF_CELLS + DSNT_ERROR_FIELD_BLOCK - 1) / DSNT_ERROR_FIELD_BLOCK;      // cells per lane at most
static_assert(EF_CELLS <= (1 << 16), "a record holds its cell in 16 bits");
constexpr int EF_MISS = 1 << 16, EF_FINITE = 1 << 17;                                         // record: cell | flags, or -1
struct error_field_edges { double e[DSNT_ERROR_FIELD_MAX_BINS + 1]; };                        // padded with +inf behind bins
static_assert(DSNT_ERROR_FIELD_MAX_BINS % 8 == 0, "error_field_cell reads the edges eight at a time");
// Cell [by][bx] of a target inside the frame.  Along an axis: the number of edges e[1..bins] that are <= t, capped at
// bins - 1, which is e[k] <= t < e[k + 1] with the last edge closed.  t is finite and the padding is +inf, so the padding
// never counts; the index is uniform, so eight edges are one scalar load of the kernel argument, as in pckh_column.
__device__ __forceinline__ int error_field_cell(const error_field_edges& edges, double tx, double ty, int bins) {
    int kx = 0, ky = 0;
    for (int q = 0; q < bins; q += 8) {
#pragma unroll
        for (int u = 1; u <= 8; ++u) {
            const double e = edges.e[q + u];
            kx += (e <= tx) ? 1 : 0;
            ky += (e <= ty) ? 1 : 0;
        }
    }
    return min(ky, bins - 1) * bins + min(kx, bins - 1);
}
__global__ __launch_bounds__(DSNT_ERROR_FIELD_BLOCK)
void error_field_kernel(const float* __restrict__ pred, const float* __restrict__ target, const double* __restrict__ m,
                        const double* __restrict__ b, const float* __restrict__ mask, const double* __restrict__ head,
                        float thr, const error_field_edges edges, double hi, int bins, long long* counts, double* sums,
                        int B, int J) {
    __shared__ int rec[DSNT_ERROR_FIELD_BLOCK];
    __shared__ double rdx[DSNT_ERROR_FIELD_BLOCK], rdy[DSNT_ERROR_FIELD_BLOCK];
    constexpr int BLOCK = DSNT_ERROR_FIELD_BLOCK;
    const int j = blockIdx.x, tid = threadIdx.x, cells = bins * bins;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t plane = (size_t)J * cells;                    // one plane of either table
    const size_t base = (size_t)j * cells;
    const double lo = edges.e[0];
    unsigned total[EF_OWN], miss[EF_OWN], finite[EF_OWN];      // this call's counts: fewer than 2^31 samples
    double sx[EF_OWN], sy[EF_OWN];                             // the table's own value, then + dx in ascending n
#pragma unroll
    for (int q = 0; q < EF_OWN; ++q) {
        const int c = tid + q * BLOCK;
        total[q] = miss[q] = finite[q] = 0u;
        sx[q] = c < cells ? sums[base + c] : 0.0;
        sy[q] = c < cells ? sums[plane + base + c] : 0.0;
    }
    for (long n0 = 0; n0 < B; n0 += BLOCK) {
        const long n = n0 + tid;
        int r = -1;                                            // records past B read as "no cell"
        double dx = 0.0, dy = 0.0;
        if (n < B) {
            const long i = n * J + j;
            const double tx = target[2 * i], ty = target[2 * i + 1];
            // mask == 1 and the target inside the closed frame (investigate.py:73-74); a NaN target fails the comparison
            if (mask[i] == 1.f && lo <= tx && tx <= hi && lo <= ty && ty <= hi) {
                r = error_field_cell(edges, tx, ty, bins);
                const double d = pckh_distance(pred, target, m, b, head, i, n);
                if (!(d <= (double)thr)) {                     // NaN and inf distances are misses, as in dsnt_pckh
                    r |= EF_MISS;
                    dx = (double)pred[2 * i] - tx;
                    dy = (double)pred[2 * i + 1] - ty;
                    if (dx - dx == 0.0 && dy - dy == 0.0) r |= EF_FINITE;      // both finite
                }
            }
        }
        rec[tid] = r;
        rdx[tid] = dx;
        rdy[tid] = dy;
        __syncthreads();
        if (wave * 64 < cells) {                               // (a wave whose lanes own no cell has nothing to scan for)
            const int len = B - n0 < BLOCK ? (int)(B - n0) : BLOCK;
            for (int s0 = 0; s0 < len; s0 += 64) {
                // 64 records, one per lane, and a ballot of those whose cell belongs to a lane of this wave; its bits are
                // walked in ascending order, which is ascending n.  A record comes out of its lane as a scalar, so the
                // branches on it are taken by the whole wave and only the owner's compare is per lane.
                const int rv = rec[s0 + lane];
                const double rx = rdx[s0 + lane], ry = rdy[s0 + lane];
                unsigned long long todo = __ballot(rv >= 0 && (((rv & 0xffff) % BLOCK) >> 6) == wave);
                while (todo) {
                    const int k = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int v = __builtin_amdgcn_readlane(rv, k);
                    const int c = v & 0xffff, slot = c / BLOCK;
                    const bool mine = tid == c % BLOCK;
                    double ax = 0.0, ay = 0.0;
                    if (v & EF_FINITE) {
                        ax = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(rx), k),
                                              __builtin_amdgcn_readlane(__double2loint(rx), k));
                        ay = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(ry), k),
                                              __builtin_amdgcn_readlane(__double2loint(ry), k));
                    }
#pragma unroll
                    for (int q = 0; q < EF_OWN; ++q) {
                        if (slot != q) continue;
                        total[q] += mine ? 1u : 0u;
                        miss[q] += (mine && (v & EF_MISS)) ? 1u : 0u;
                        if (v & EF_FINITE) {
                            finite[q] += mine ? 1u : 0u;
                            if (mine) {
                                sx[q] += ax;
                                sy[q] += ay;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < EF_OWN; ++q) {
        const int c = tid + q * BLOCK;
        if (c < cells) {
            counts[base + c] += (long long)total[q];
            counts[plane + base + c] += (long long)miss[q];
            counts[2 * plane + base + c] += (long long)finite[q];
            sums[base + c] = sx[q];
            sums[plane + base + c] = sy[q];
        }
    }
}
extern "C" int dsnt_error_field(const float* pred, const float* target, const double* m, const double* b,
                                const float* mask, const double* head, float threshold, const double* edges, int bins,
                                int64_t* counts, double* sums, int B, int J, void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && edges && counts && sums && B > 0 && J > 0,
                 DSNT_ERR_ARG, "dsnt_error_field: bad argument");
    DSNT_REQUIRE(bins >= 1 && bins <= DSNT_ERROR_FIELD_MAX_BINS, DSNT_ERR_ARG, "dsnt_error_field: bins=%d outside 1..%d",
                 bins, DSNT_ERROR_FIELD_MAX_BINS);
    error_field_edges e;
    if (const int rc = ascending_arg("dsnt_error_field", "edge", edges, bins + 1, e.e)) return rc;
    const double hi = e.e[bins];
    DSNT_LAUNCH(error_field_kernel, dim3(J), dim3(DSNT_ERROR_FIELD_BLOCK), 0, (hipStream_t)stream, pred, target, m, b,
                mask, head, threshold, e, hi, bins, (long long*)counts, sums, B, J);
    DSNT_CHECK_LAUNCH("dsnt_error_field");
}

// ---------------------------------------------------------------- what kind of miss
// What dsnt_joint_confusion and dsnt_target_mass refuse alike, and the mirror as their kernels take it: by value, a byte
// per joint, checked here on the host.  0 or the error code; nothing has touched a device.
struct joint_mirror { unsigned char p[DSNT_CONFUSION_MAX_J]; };
static_assert(DSNT_CONFUSION_MAX_J < 255, "a joint fits a byte, 255 marks a joint that does not count");
static int confusion_args(const char* who, bool pointers, int B, int J, float threshold, const int* mirror,
                          joint_mirror& out) {
    DSNT_REQUIRE(pointers, DSNT_ERR_ARG, "%s: null pointer", who);
    DSNT_REQUIRE(B > 0, DSNT_ERR_ARG, "%s: B=%d out of range", who, B);
    DSNT_REQUIRE(J >= 1 && J <= DSNT_CONFUSION_MAX_J, DSNT_ERR_ARG, "%s: J=%d outside 1..%d", who, J,
                 DSNT_CONFUSION_MAX_J);
    DSNT_REQUIRE(threshold >= 0.f && threshold - threshold == 0.f, DSNT_ERR_ARG,
                 "%s: threshold %g is negative or not finite", who, (double)threshold);
    for (int j = 0; j < DSNT_CONFUSION_MAX_J; ++j) out.p[j] = (unsigned char)j;
    for (int j = 0; j < J; ++j) {
        DSNT_REQUIRE(mirror[j] >= 0 && mirror[j] < J && mirror[mirror[j]] == j, DSNT_ERR_ARG,
                     "%s: mirror is not an involution of 0..%d (mirror[%d] = %d)", who, J - 1, j, mirror[j]);
        out.p[j] = (unsigned char)mirror[j];
    }
    return DSNT_OK;
}

// Joint confusion (include/dsnt_hip.h: dsnt_joint_confusion): every counted joint adds 1 to one cell of table[J][J + 1],
// the joint whose target its prediction landed on (its own: the hit of pckh_kernel) or column J for none, and mutual[J]
// counts the mirrored pairs that landed on each other.  Integer adds only, so the tables do not depend on the order of
// arrival, nor on how the examples are batched.  The unit of work is the person: a pass of a workgroup takes
// BLOCK / J of them, thread (p, j) back-projects target j of person p into LDS once, then holds its prediction against the
// person's J targets there, and leaves its cell in LDS for its mirror to read.  At most DSNT_CONFUSION_MAX_BLOCKS
// workgroups stride over the persons; each counts in a u32 LDS copy [J][J + 2] (the table's columns, then mutual: a cell
// takes at most one from each person) and flushes its non-zero cells with one 64-bit atomic each.
static_assert(DSNT_CONFUSION_BLOCK >= DSNT_CONFUSION_MAX_J && DSNT_CONFUSION_BLOCK % 64 == 0,
              "a pass holds at least one person");
__global__ __launch_bounds__(DSNT_CONFUSION_BLOCK)
void joint_confusion_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                            const double* __restrict__ m, const double* __restrict__ b, const float* __restrict__ mask,
                            const double* __restrict__ head, float thr, const joint_mirror mirror,
                            unsigned long long* table, unsigned long long* mutual, int B, int J) {
    constexpr int BLOCK = DSNT_CONFUSION_BLOCK, NONE = 255;
    __shared__ unsigned cnt[DSNT_CONFUSION_MAX_J * (DSNT_CONFUSION_MAX_J + 2)];
    __shared__ double gx[BLOCK], gy[BLOCK];                    // the back-projected targets of this pass
    __shared__ unsigned char ann[BLOCK], cell[BLOCK];          // target annotated (mask == 1); the joint's column, or NONE
    __shared__ unsigned char mir[DSNT_CONFUSION_MAX_J];
    const int tid = threadIdx.x, stride = J + 2, cells = J * stride;
    const int per = BLOCK / J;                                 // persons of a pass
    const int p = tid / J, j = tid - p * J, base = p * J;      // this thread's person of the pass, joint, and slot of joint 0
    const double t = (double)thr;
    for (int c = tid; c < cells; c += BLOCK) cnt[c] = 0u;
    if (tid < J) mir[tid] = mirror.p[tid];
    for (long n0 = (long)blockIdx.x * per; n0 < B; n0 += (long)gridDim.x * per) {
        __syncthreads();                                       // the zeroes above, and the last pass's readers of cell
        const long n = n0 + p;
        bool counted = false;
        pckh_point o = {0.0, 0.0};
        double hd = 1.0;
        if (p < per && n < B) {
            const long i = n * J + j;
            const double* mm = m + (size_t)n * 4;
            const double* bb = b + (size_t)n * 2;
            const pckh_point g = pckh_project(target[2 * i], target[2 * i + 1], mm, bb);
            gx[tid] = g.x;
            gy[tid] = g.y;
            counted = mask[i] == 1.f;
            ann[tid] = counted ? 1 : 0;
            o = pckh_project(pred[2 * i], pred[2 * i + 1], mm, bb);
            hd = head[n];
        }
        __syncthreads();
        int c = NONE;
        if (counted) {
            c = J;                                             // no comparison holds for a NaN: it stays here
            if (pckh_between(o, {gx[tid], gy[tid]}, hd) <= t) {
                c = j;
            } else {
                double best = (double)INFINITY;
                for (int k = 0; k < J; ++k) {                  // ascending k and a strict <: an exact tie keeps the smaller
                    if (k == j || !ann[base + k]) continue;
                    const double d = pckh_between(o, {gx[base + k], gy[base + k]}, hd);
                    if (d <= t && d < best) {
                        best = d;
                        c = k;
                    }
                }
            }
            atomicAdd(cnt + j * stride + c, 1u);
        }
        cell[tid] = (unsigned char)c;
        __syncthreads();
        if (counted) {
            const int mj = mir[j];                             // (a partner that is not counted holds NONE, never j)
            if (mj != j && c == mj && cell[base + mj] == j) atomicAdd(cnt + j * stride + J + 1, 1u);
        }
    }
    __syncthreads();
    for (int c = tid; c < cells; c += BLOCK) {
        const unsigned v = cnt[c];
        if (!v) continue;
        const int row = c / stride, col = c - row * stride;
        if (col <= J) atomicAdd(table + row * (J + 1) + col, (unsigned long long)v);
        else atomicAdd(mutual + row, (unsigned long long)v);
    }
}
extern "C" int dsnt_joint_confusion(const float* pred, const float* target, const double* m, const double* b,
                                    const float* mask, const double* head, float threshold, const int* mirror,
                                    unsigned long long* table, unsigned long long* mutual, int B, int J, void* stream) {
    joint_mirror mir;
    if (const int rc = confusion_args("dsnt_joint_confusion", pred && target && m && b && mask && head && mirror && table &&
                                      mutual, B, J, threshold, mirror, mir)) return rc;
    const int per = DSNT_CONFUSION_BLOCK / J;
    const long want = ((long)B + per - 1) / per;
    const int grid = (int)(want < DSNT_CONFUSION_MAX_BLOCKS ? want : DSNT_CONFUSION_MAX_BLOCKS);
    DSNT_LAUNCH(joint_confusion_kernel, dim3(grid), dim3(DSNT_CONFUSION_BLOCK), 0, (hipStream_t)stream, pred, target, m, b,
                mask, head, threshold, mir, table, mutual, B, J);
    DSNT_CHECK_LAUNCH("dsnt_joint_confusion");
}

// Heat-map mass at the target (include/dsnt_hip.h: dsnt_target_mass): one workgroup per row (n, j) sums the pixels of
// hm[n][j] whose centre, back-projected, lies within the threshold of the joint's target, and of its mirror's target.
// Thread t takes the pixels 4q .. 4q + 3 for q = t, t + BLOCK, ... in ascending order, one 16-byte load each with VEC4
// and four scalar loads without, so both forms add the same numbers in the same order: fp64 partial sums per thread,
// the xor tree across the wave, then the waves in ascending order.  Every pixel is tested: no bounding box.
static_assert(DSNT_TARGET_MASS_BLOCK % 64 == 0 && DSNT_TARGET_MASS_BLOCK >= 64, "whole waves");
template <bool VEC4>
__global__ __launch_bounds__(DSNT_TARGET_MASS_BLOCK)
void target_mass_kernel(const float* __restrict__ hm, const float* __restrict__ target, const double* __restrict__ m,
                        const double* __restrict__ b, const float* __restrict__ mask, const double* __restrict__ head,
                        float thr, const joint_mirror mirror, float* __restrict__ out, int J, int h, int w) {
    constexpr int BLOCK = DSNT_TARGET_MASS_BLOCK, WAVES = BLOCK / 64;
    __shared__ double red[2 * WAVES];
    const int tid = threadIdx.x;
    const long row = blockIdx.x, n = row / J;
    const int j = (int)(row - n * J);
    if (!(mask[row] == 1.f)) {                                 // the same for every thread of the row
        if (tid == 0) out[2 * row] = out[2 * row + 1] = NAN;
        return;
    }
    const int mj = mirror.p[j];
    const long partner = n * J + mj;
    const bool two = mj != j && mask[partner] == 1.f;
    const double* mm = m + (size_t)n * 4;
    const double* bb = b + (size_t)n * 2;
    const pckh_point g = pckh_project(target[2 * row], target[2 * row + 1], mm, bb);
    const pckh_point gm = pckh_project(target[2 * partner], target[2 * partner + 1], mm, bb);      // (unused unless `two`)
    const double hd = head[n], t = (double)thr, dw = (double)w, dh = (double)h;
    const int hw = h * w, groups = (hw + 3) >> 2;
    const float* __restrict__ px = hm + (size_t)row * hw;
    double s0 = 0.0, s1 = 0.0;
    for (int q = tid; q < groups; q += BLOCK) {
        const int i0 = 4 * q;
        float v[4];
        if (VEC4) {
            const float4 f = *reinterpret_cast<const float4*>(px + i0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = i0 + u < hw ? px[i0 + u] : 0.f;
        }
        int r = i0 / w, c = i0 - r * w;
        double y = (double)(2 * r + 1 - h) / dh;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!VEC4 && i0 + u >= hw) break;
            const double x = (double)(2 * c + 1 - w) / dw;     // the centre of pixel (r, c) on dsnt.nn.generate_xy's grid
            const pckh_point o = pckh_project(x, y, mm, bb);
            if (pckh_between(o, g, hd) <= t) s0 += (double)v[u];
            if (two && pckh_between(o, gm, hd) <= t) s1 += (double)v[u];
            ++c;
            if (!VEC4 && c == w) {                             // (w % 4 == 0 with VEC4: the four share a row)
                c = 0;
                y = (double)(2 * ++r + 1 - h) / dh;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
    }
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = s0;
        red[2 * (tid >> 6) + 1] = s1;
    }
    __syncthreads();
    if (tid == 0) {
        s0 = red[0];
        s1 = red[1];
        for (int wv = 1; wv < WAVES; ++wv) {
            s0 += red[2 * wv];
            s1 += red[2 * wv + 1];
        }
        out[2 * row] = (float)s0;
        out[2 * row + 1] = two ? (float)s1 : NAN;
    }
}
extern "C" int dsnt_target_mass(const float* heatmaps, const float* target, const double* m, const double* b,
                                const float* mask, const double* head, float threshold, const int* mirror, float* out,
                                int B, int J, int h, int w, void* stream) {
    joint_mirror mir;
    if (const int rc = confusion_args("dsnt_target_mass", heatmaps && target && m && b && mask && head && mirror && out, B, J,
                                      threshold, mirror, mir)) return rc;
    DSNT_REQUIRE((long)B * J < (1L << 31), DSNT_ERR_ARG, "dsnt_target_mass: B=%d out of range", B);
    DSNT_REQUIRE(h > 0 && w > 0 && (long)h * w < (1L << 24), DSNT_ERR_SHAPE, "dsnt_target_mass: bad map size %dx%d", h, w);
    const dim3 grid((unsigned)(B * J)), block(DSNT_TARGET_MASS_BLOCK);
    if (w % 4 == 0 && dsnt_aligned16(heatmaps))
        DSNT_LAUNCH(target_mass_kernel<true>, grid, block, 0, (hipStream_t)stream, heatmaps, target, m, b, mask, head,
                    threshold, mir, out, J, h, w);
    else
        DSNT_LAUNCH(target_mass_kernel<false>, grid, block, 0, (hipStream_t)stream, heatmaps, target, m, b, mask, head,
                    threshold, mir, out, J, h, w);
    DSNT_CHECK_LAUNCH("dsnt_target_mass");
}
