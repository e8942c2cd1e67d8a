// Importance-sampled epochs (include/dsnt_hip.h: dsnt_sample_cdf, dsnt_sample_indices, dsnt_example_scores;
// dsnt.data.ExampleScores, WeightedLoader).  Restated in numpy by tests/sampler_ref.py.
//
// dsnt_sample_cdf: an exact fixed-point CDF over fp32 row weights.  A weight counts if its bit pattern is that of a
// positive finite float (0 < bits < 0x7F800000: NaN, +-inf, negatives and both zeros fail an integer compare, and a
// subnormal counts whatever the denormal mode).  wmax = the largest counted weight = f 2^e with f in [0.5, 1);
// q[i] = floor(w[i] 2^(32 - e)) < 2^32, taken from the weight's own mantissa and exponent by a shift, so no rounding
// happens anywhere; cdf[i] = q[0] + .. + q[i] in u64 (< 2^56: exact, and the same in any order of summation).  Five
// stream-ordered launches: the scratch's maximum word is zeroed; an integer atomic max over the bit patterns (for
// non-negative floats bit order is value order, so the result does not depend on arrival); a scan of every tile of
// SAMPLE_TILE weights inside its workgroup, which also leaves the tile's total in the scratch; one workgroup scans the
// totals (at most 2^24 / SAMPLE_TILE = 16384 of them); every tile adds its offset.  No workgroup ever waits on another of
// its launch: the launch boundaries are the only ordering.
//
// dsnt_sample_indices: position p of an epoch draws u = o0 2^32 + o1 from Philox4x32-10 keyed by seed with counter
// (p, epoch lo, epoch hi, DSNT_SAMPLE_DOMAIN), t = floor(u T / 2^64) with T = cdf[n - 1], and takes the smallest j with
// cdf[j] > t by bisection (t < T, so there is one; a row with q == 0 has cdf[j] == cdf[j - 1] and is never the smallest).
//
// dsnt_example_scores: one thread per example sums pckh_distance over its counted joints in joint order in fp64, and
// leaves (stamp << 32) | bits(score) in the table by one 64-bit atomic max.  Not a hot kernel: B threads, J loads each.
#include "common.h"
#include "philox.h"
#include "pckh_dist.h"

namespace {

constexpr int SAMPLE_NT = 256;
constexpr int SAMPLE_PER = DSNT_SAMPLE_TILE / SAMPLE_NT;      // consecutive weights of a thread
static_assert(DSNT_SAMPLE_TILE == SAMPLE_NT * SAMPLE_PER && SAMPLE_NT % 64 == 0, "a tile is whole waves of whole threads");
constexpr int SAMPLE_MAX_TILES = (int)(((int64_t)DSNT_SAMPLE_MAX_N + DSNT_SAMPLE_TILE - 1) / DSNT_SAMPLE_TILE);
constexpr int SAMPLE_MAX_GRID = 1024;                          // workgroups of the grid-stride maximum

__device__ __forceinline__ bool sample_counts(uint32_t bits) { return bits != 0u && bits < 0x7F800000u; }

// frexp's exponent of a counted weight from its bits: value = f 2^e, f in [0.5, 1).
__device__ __forceinline__ int sample_exponent(uint32_t bits) {
    const int E = (int)(bits >> 23);
    if (E) return E - 126;                                     // 1.m 2^(E - 127) = 0.1m 2^(E - 126)
    return (31 - __clz((int)bits)) - 148;                      // subnormal: m 2^-149, top bit h: [2^(h - 149), 2^(h - 148))
}
// floor(w 2^(32 - e)) for a counted weight w <= wmax < 2^e: w = M 2^X with M its 24-bit significand, shifted.
__device__ __forceinline__ uint64_t sample_quantise(uint32_t bits, int e) {
    if (!sample_counts(bits)) return 0ull;
    const int E = (int)(bits >> 23);
    const uint64_t M = E ? (uint64_t)((bits & 0x7FFFFFu) | 0x800000u) : (uint64_t)bits;
    const int s = (E ? E - 150 : -149) + 32 - e;               // w < 2^e: M 2^s < 2^32
    if (s >= 0) return M << s;
    return s > -24 ? M >> -s : 0ull;
}

__global__ void sample_init_kernel(uint32_t* __restrict__ wmax) {
    wmax[0] = 0u;
    wmax[1] = 0u;
}

__global__ void __launch_bounds__(SAMPLE_NT) sample_max_kernel(const uint32_t* __restrict__ w, int64_t n,
                                                               uint32_t* __restrict__ wmax) {
    __shared__ uint32_t red[SAMPLE_NT / 64];
    uint32_t m = 0u;
    for (int64_t i = (int64_t)blockIdx.x * SAMPLE_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * SAMPLE_NT) {
        const uint32_t b = w[i];
        if (sample_counts(b) && b > m) m = b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SAMPLE_NT / 64; ++k) m = red[k] > m ? red[k] : m;
        if (m) atomicMax(wmax, m);
    }
}

// Inclusive scan of one u64 per thread across the workgroup (SAMPLE_NT threads); `red` holds a word per wave.  Returns the
// thread's inclusive sum; *total (if given) gets the workgroup's.
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t v, uint64_t* red, uint64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
        if (lane >= o) v += up;
    }
    __syncthreads();                                           // a previous use of red
    if (lane == 63) red[wave] = v;
    __syncthreads();
    uint64_t before = 0ull, all = 0ull;
#pragma unroll
    for (int k = 0; k < SAMPLE_NT / 64; ++k) {
        const uint64_t r = red[k];
        if (k < wave) before += r;
        all += r;
    }
    if (total) *total = all;
    return v + before;
}

// Tile blockIdx.x: cdf[i] = the sum of q over the tile up to i; totals[tile] = the tile's sum.
__global__ void __launch_bounds__(SAMPLE_NT) sample_scan_tiles_kernel(const uint32_t* __restrict__ w, int64_t n,
                                                                      const uint32_t* __restrict__ wmax,
                                                                      uint64_t* __restrict__ cdf,
                                                                      uint64_t* __restrict__ totals) {
    __shared__ uint64_t red[SAMPLE_NT / 64];
    const uint32_t top = wmax[0];
    const int e = top ? sample_exponent(top) : 0;              // (top == 0: nothing counts, every q is 0)
    const int64_t i0 = (int64_t)blockIdx.x * DSNT_SAMPLE_TILE + (int64_t)threadIdx.x * SAMPLE_PER;
    uint64_t q[SAMPLE_PER], sum = 0ull;
#pragma unroll
    for (int k = 0; k < SAMPLE_PER; ++k) {
        q[k] = i0 + k < n ? sample_quantise(w[i0 + k], e) : 0ull;
        sum += q[k];
    }
    uint64_t all;
    uint64_t run = block_scan_u64(sum, red, &all) - sum;       // the sum of the threads before this one
#pragma unroll
    for (int k = 0; k < SAMPLE_PER; ++k) {
        run += q[k];
        if (i0 + k < n) cdf[i0 + k] = run;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = all;
}

// One workgroup: totals[t] becomes the sum of the totals before tile t.  Thread k owns `per` consecutive tiles.
__global__ void __launch_bounds__(SAMPLE_NT) sample_scan_totals_kernel(uint64_t* __restrict__ totals, int tiles, int per) {
    __shared__ uint64_t red[SAMPLE_NT / 64];
    const int t0 = threadIdx.x * per, t1 = min(t0 + per, tiles);
    uint64_t sum = 0ull;
    for (int t = t0; t < t1; ++t) sum += totals[t];
    uint64_t run = block_scan_u64(sum, red, nullptr) - sum;
    for (int t = t0; t < t1; ++t) {
        const uint64_t v = totals[t];
        totals[t] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(SAMPLE_NT) sample_add_offsets_kernel(uint64_t* __restrict__ cdf, int64_t n,
                                                                       const uint64_t* __restrict__ offsets) {
    const uint64_t off = offsets[blockIdx.x];
    const int64_t i0 = (int64_t)blockIdx.x * DSNT_SAMPLE_TILE + threadIdx.x;
#pragma unroll
    for (int k = 0; k < SAMPLE_PER; ++k) {
        const int64_t i = i0 + (int64_t)k * SAMPLE_NT;
        if (i < n) cdf[i] += off;
    }
}

__global__ void __launch_bounds__(SAMPLE_NT) sample_indices_kernel(const uint64_t* __restrict__ cdf, int64_t n, uint64_t seed,
                                                                   uint64_t epoch, int64_t first, int64_t count,
                                                                   int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SAMPLE_NT + threadIdx.x;
    if (i >= count) return;
    const uint64_t T = cdf[n - 1];
    if (T == 0ull) {
        out[i] = -1;
        return;
    }
    uint32_t o[4];
    Philox::gen(o, seed, epoch, (uint32_t)(uint64_t)(first + i), DSNT_SAMPLE_DOMAIN);
    const uint64_t t = __umul64hi(((uint64_t)o[0] << 32) | o[1], T);      // < T
    int64_t lo = 0, hi = n - 1;                                // cdf[hi] > t throughout
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    out[i] = lo;
}

__global__ void __launch_bounds__(SAMPLE_NT) example_scores_kernel(const float* __restrict__ pred,
                                                                   const float* __restrict__ target,
                                                                   const double* __restrict__ m, const double* __restrict__ b,
                                                                   const float* __restrict__ mask,
                                                                   const double* __restrict__ head,
                                                                   const int64_t* __restrict__ idx, int64_t N, uint32_t stamp,
                                                                   unsigned long long* table, float* __restrict__ score,
                                                                   int B, int J) {
    const int n = blockIdx.x * SAMPLE_NT + threadIdx.x;
    if (n >= B) return;
    double sum = 0.0;
    int cnt = 0;
    for (int j = 0; j < J; ++j) {
        const long i = (long)n * J + j;
        if (!(mask[i] == 1.f)) continue;
        sum += pckh_distance(pred, target, m, b, head, i, n);
        ++cnt;
    }
    const float s = cnt ? (float)(sum / (double)cnt) : NAN;
    score[n] = s;
    const uint32_t bits = __float_as_uint(s);
    const int64_t row = idx[n];
    if ((bits & 0x7F800000u) != 0x7F800000u && row >= 0 && row < N)
        atomicMax(table + row, ((unsigned long long)stamp << 32) | bits);
}

}  // namespace

extern "C" int dsnt_sample_cdf(const float* weights, int64_t n, uint64_t* cdf, void* scratch, void* stream) {
    DSNT_REQUIRE(weights && cdf && scratch, DSNT_ERR_ARG, "dsnt_sample_cdf: null pointer");
    DSNT_REQUIRE(n >= 1 && n <= DSNT_SAMPLE_MAX_N, DSNT_ERR_SHAPE, "dsnt_sample_cdf: n=%lld outside 1..%lld", (long long)n,
                 (long long)DSNT_SAMPLE_MAX_N);
    const int tiles = (int)((n + DSNT_SAMPLE_TILE - 1) / DSNT_SAMPLE_TILE);            // <= SAMPLE_MAX_TILES
    static_assert(SAMPLE_MAX_TILES <= SAMPLE_NT * 64, "a thread of the totals scan owns at most 64 tiles");
    uint32_t* wmax = (uint32_t*)scratch;                       // the first 8 bytes; the tile totals follow
    uint64_t* totals = (uint64_t*)scratch + 1;
    const uint32_t* bits = (const uint32_t*)weights;
    const hipStream_t s = (hipStream_t)stream;
    DSNT_LAUNCH(sample_init_kernel, dim3(1), dim3(1), 0, s, wmax);
    DSNT_LAUNCH(sample_max_kernel, dim3(tiles < SAMPLE_MAX_GRID ? tiles : SAMPLE_MAX_GRID), dim3(SAMPLE_NT), 0, s, bits, n,
                wmax);
    DSNT_LAUNCH(sample_scan_tiles_kernel, dim3(tiles), dim3(SAMPLE_NT), 0, s, bits, n, (const uint32_t*)wmax, cdf, totals);
    DSNT_LAUNCH(sample_scan_totals_kernel, dim3(1), dim3(SAMPLE_NT), 0, s, totals, tiles, (tiles + SAMPLE_NT - 1) / SAMPLE_NT);
    DSNT_LAUNCH(sample_add_offsets_kernel, dim3(tiles), dim3(SAMPLE_NT), 0, s, cdf, n, (const uint64_t*)totals);
    DSNT_CHECK_LAUNCH("dsnt_sample_cdf");
}

extern "C" int dsnt_sample_indices(const uint64_t* cdf, int64_t n, uint64_t seed, uint64_t epoch, int64_t first,
                                   int64_t count, int64_t* out, void* stream) {
    DSNT_REQUIRE(cdf && out, DSNT_ERR_ARG, "dsnt_sample_indices: null pointer");
    DSNT_REQUIRE(n >= 1 && n <= DSNT_SAMPLE_MAX_N, DSNT_ERR_SHAPE, "dsnt_sample_indices: n=%lld outside 1..%lld",
                 (long long)n, (long long)DSNT_SAMPLE_MAX_N);
    DSNT_REQUIRE(first >= 0 && first < (1LL << 32) && count > 0 && count <= (1LL << 32) - first, DSNT_ERR_SHAPE,
                 "dsnt_sample_indices: bad range first=%lld count=%lld (positions lie in [0, 2^32))", (long long)first,
                 (long long)count);
    DSNT_LAUNCH(sample_indices_kernel, dim3((unsigned)((count + SAMPLE_NT - 1) / SAMPLE_NT)), dim3(SAMPLE_NT), 0,
                (hipStream_t)stream, cdf, n, seed, epoch, first, count, out);
    DSNT_CHECK_LAUNCH("dsnt_sample_indices");
}

extern "C" int dsnt_example_scores(const float* pred, const float* target, const double* m, const double* b,
                                   const float* mask, const double* head, const int64_t* idx, int64_t N, uint32_t stamp,
                                   unsigned long long* table, float* score, int B, int J, void* stream) {
    DSNT_REQUIRE(pred && target && m && b && mask && head && idx && table && score && B > 0 && J > 0, DSNT_ERR_ARG,
                 "dsnt_example_scores: bad argument");
    DSNT_REQUIRE(N >= 1, DSNT_ERR_ARG, "dsnt_example_scores: N=%lld out of range", (long long)N);
    DSNT_REQUIRE(stamp >= 1u && stamp < 0x80000000u, DSNT_ERR_ARG, "dsnt_example_scores: stamp %u outside [1, 2^31)", stamp);
    DSNT_LAUNCH(example_scores_kernel, dim3((B + SAMPLE_NT - 1) / SAMPLE_NT), dim3(SAMPLE_NT), 0, (hipStream_t)stream, pred,
                target, m, b, mask, head, idx, N, stamp, table, score, B, J);
    DSNT_CHECK_LAUNCH("dsnt_example_scores");
}
