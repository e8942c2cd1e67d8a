// Mode-seeking read-out of heat-maps (include/dsnt_hip.h: dsnt_map_modes): the K dominant modes of a
// map as window centroids, where the DSNT expectation of a bimodal map lands between its modes.
//
// One 256-thread workgroup per row (one map p[h][w], used as given).  The row is staged in LDS plane A; the horizontal
// pass writes the (2r+1)-pixel row sums s into plane B, the vertical pass writes the window scores S back over plane A.
// Thread t owns the pixels t, t + 256, ... of the flat map (row-major), so for every offset d of either pass the lanes of
// a wave read consecutive LDS addresses: no bank conflicts.  Every add of the two passes is a separately rounded fp32
// add in ascending d from +0, a pixel outside the map adding +0 (never a sliding window: it rounds differently).  This
// file is compiled with -ffp-contract=off (build.py).
//
// K rounds of workgroup arg-max over S follow (value, then smallest index: block_peak's idiom, flipmerge.h, with -1 for
// "no winner"); plane B is dead by then and holds the reduction's four floats.  Wave k then sums mode k's window in fp64
// from the map in global memory (at most 17 x 17 pixels, L2-resident): lane l takes window row yc - r + l in ascending x,
// lane 0 adds the rows that lie in the map in ascending y, and writes the mode with plain stores.
#include "common.h"
#include <math.h>

#define MB 256   // threads per row: four waves, one per mode in the last phase (K <= DSNT_MODES_MAX_K = 4)
static_assert(MB / DSNT_WAVE >= DSNT_MODES_MAX_K, "one wave per mode");

struct ModesOut {
    float* coords;
    float* mass;
    int* index;
    double* image;
};

template <bool VEC4>
__global__ __launch_bounds__(MB) void map_modes_kernel(const float* __restrict__ hm, int J, int h, int w, int r, int K,
                                                       const double* __restrict__ tm, const double* __restrict__ tb,
                                                       ModesOut o) {
    extern __shared__ __align__(16) float planes[];
    const int hw = h * w, tid = threadIdx.x;
    float* A = planes;                        // p, then S
    float* Bp = planes + ((hw + 3) & ~3);     // s, then the reductions' scratch
    const size_t row = blockIdx.x;
    const float* p = hm + row * (size_t)hw;

    if (VEC4) {       // w % 4 == 0 and a 16-byte aligned base: every row of the tensor is aligned
        for (int q = tid; q < hw / 4; q += MB)
            reinterpret_cast<float4*>(A)[q] = reinterpret_cast<const float4*>(p)[q];
    } else {
        for (int i = tid; i < hw; i += MB) A[i] = p[i];
    }
    __syncthreads();
    for (int i = tid; i < hw; i += MB) {
        const int y = i / w, x = i - y * w;
        float acc = 0.f;
        for (int d = -r; d <= r; ++d) acc += (x + d >= 0 && x + d < w) ? A[i + d] : 0.f;
        Bp[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < hw; i += MB) {
        const int y = i / w;
        float acc = 0.f;
        for (int d = -r; d <= r; ++d) acc += (y + d >= 0 && y + d < h) ? Bp[i + d * w] : 0.f;
        A[i] = acc;
    }
    __syncthreads();

    // mode k: the first largest S among the centres further than 2r (Chebyshev) from every earlier centre
    float* red = Bp;
    int ci[DSNT_MODES_MAX_K], cy[DSNT_MODES_MAX_K], cx[DSNT_MODES_MAX_K];
#pragma unroll
    for (int k = 0; k < DSNT_MODES_MAX_K; ++k) {
        ci[k] = -1; cy[k] = 0; cx[k] = 0;
        if (k >= K) continue;
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < hw; i += MB) {
            const float s = A[i];
            if (s > best) {                   // ascending i per thread: keeps the first maximum; a NaN never wins
                const int y = i / w, x = i - y * w;
                bool far = true;
#pragma unroll
                for (int j = 0; j < k; ++j)
                    far = far && (ci[j] < 0 || max(abs(y - cy[j]), abs(x - cx[j])) > 2 * r);
                if (far) { best = s; bi = i; }
            }
        }
        const float m = block_max(best, red);
        const float cand = (bi != 0x7fffffff && best == m) ? (float)bi : 16777216.f;      // indices < 2^13: exact
        const float first = -block_max(-cand, red);
        if (first < 16777216.f) {
            ci[k] = (int)first;
            cy[k] = ci[k] / w;
            cx[k] = ci[k] - cy[k] * w;
        }
    }

    const int lane = tid & 63, k = tid >> 6;
    if (k >= K) return;
    int c = -1;
#pragma unroll
    for (int j = 0; j < DSNT_MODES_MAX_K; ++j)
        if (j == k) c = ci[j];
    const int yc = c < 0 ? 0 : c / w, xc = c < 0 ? 0 : c - yc * w;
    double sm = 0.0, sx = 0.0, sy = 0.0;
    const int yy = yc - r + lane;
    if (c >= 0 && lane <= 2 * r && yy >= 0 && yy < h) {
        const double Y = (double)(2 * yy + 1) / (double)h - 1.0;
        for (int xx = max(0, xc - r); xx <= min(w - 1, xc + r); ++xx) {
            const double v = (double)p[yy * w + xx];
            const double X = (double)(2 * xx + 1) / (double)w - 1.0;
            sm += v;
            sx += X * v;
            sy += Y * v;
        }
    }
    double tot = 0.0, totx = 0.0, toty = 0.0;
    for (int l = 0; l <= 2 * r; ++l) {
        const double a = __shfl(sm, l, 64), b = __shfl(sx, l, 64), d = __shfl(sy, l, 64);
        if (yc - r + l >= 0 && yc - r + l < h) { tot += a; totx += b; toty += d; }
    }
    if (lane != 0) return;
    const float nan = __int_as_float(0x7fc00000);
    float mass = nan, fx = nan, fy = nan;
    if (c >= 0) {
        mass = (float)tot;
        if (tot > 0.0) { fx = (float)(totx / tot); fy = (float)(toty / tot); }
    }
    const size_t slot = row * (size_t)K + k;
    o.index[slot] = c;
    o.mass[slot] = mass;
    o.coords[2 * slot] = fx;
    o.coords[2 * slot + 1] = fy;
    if (o.image) {      // predict's convention: img = t + c . M on row vectors, from the f32-rounded coordinates
        const double* M = tm + 4 * (row / (size_t)J);
        const double* t = tb + 2 * (row / (size_t)J);
        const double x = fx, y = fy;
        o.image[2 * slot] = t[0] + (x * M[0] + y * M[2]);
        o.image[2 * slot + 1] = t[1] + (x * M[1] + y * M[3]);
    }
}

extern "C" int dsnt_map_modes(const float* hm, int64_t rows, int J, int h, int w, int radius, int K,
                              const double* transform_m, const double* transform_b, float* coords, float* mass,
                              int* index, double* image, void* stream) {
    DSNT_REQUIRE(hm && coords && mass && index, DSNT_ERR_ARG, "dsnt_map_modes: null pointer");
    DSNT_REQUIRE(rows > 0 && rows < (1LL << 31) && J > 0 && rows % J == 0, DSNT_ERR_ARG,
                 "dsnt_map_modes: rows=%lld must be a positive multiple of J=%d below 2^31", (long long)rows, J);
    DSNT_REQUIRE(radius >= 0 && radius <= DSNT_MODES_MAX_RADIUS, DSNT_ERR_ARG, "dsnt_map_modes: radius=%d outside 0..%d",
                 radius, DSNT_MODES_MAX_RADIUS);
    DSNT_REQUIRE(K >= 1 && K <= DSNT_MODES_MAX_K, DSNT_ERR_ARG, "dsnt_map_modes: K=%d outside 1..%d", K,
                 DSNT_MODES_MAX_K);
    DSNT_REQUIRE((transform_m != nullptr) == (transform_b != nullptr) && (transform_m != nullptr) == (image != nullptr),
                 DSNT_ERR_ARG, "dsnt_map_modes: transform_m, transform_b and image must be all null or all non-null");
    DSNT_REQUIRE(h > 0 && w > 0 && (long)h * w <= DSNT_MODES_MAX_PIXELS, DSNT_ERR_SHAPE,
                 "dsnt_map_modes: map %dx%d outside 1..%d pixels (the row lives in LDS); dsnt_heatmap_stats takes larger maps",
                 h, w, DSNT_MODES_MAX_PIXELS);
    const int plane = (h * w + 3) & ~3;
    const size_t lds = (size_t)(plane + (plane > 64 ? plane : 64)) * sizeof(float);      // <= 64 KiB: no launch attribute
    const ModesOut o{coords, mass, index, image};
    const dim3 grid((unsigned)rows), block(MB);
    if (w % 4 == 0 && dsnt_aligned16(hm))
        DSNT_LAUNCH(map_modes_kernel<true>, grid, block, lds, (hipStream_t)stream, hm, J, h, w, radius, K, transform_m,
                    transform_b, o);
    else
        DSNT_LAUNCH(map_modes_kernel<false>, grid, block, lds, (hipStream_t)stream, hm, J, h, w, radius, K, transform_m,
                    transform_b, o);
    DSNT_CHECK_LAUNCH("dsnt_map_modes");
}
