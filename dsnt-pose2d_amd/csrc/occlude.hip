// Synthetic occlusion of a batch of model inputs, one launch per batch (include/dsnt_hip.h: dsnt_occlude;
// dsnt.data.Occlude).  Restated in numpy by tests/occlude_ref.py.
//
// in f32 [B][3][S][S] -> out f32 [B][3][S][S]: out = in outside the sample's rectangles, the fill inside them.  Out of
// place on purpose: the paste fill reads another sample of the same batch from `in`, which an in-place kernel might
// already have overwritten with that sample's own occlusion; with a second tensor there is no order to get wrong and
// the result is bit-reproducible.
//
// The draw (draw != 0), integers only.  u24(x) = x >> 8; pick(x, n) = (u24(x) * n) >> 24 in 64 bits, a value in [0, n).
// P(k) = Philox4x32-10 with key (seed lo, seed hi) and counter (g, step lo, step hi, DSNT_OCCLUDE_DOMAIN + k),
// g = draw_offset + b.  A = P(0): the sample is occluded iff u24(A0) < p24 (p24 = round(p 2^24)); count = 1 + pick(A1, K)
// if so, else 0; donor = (b + 1 + pick(A2, B - 1)) % B for B > 1, else b (never b itself while there is another sample).
// Rectangle r < count, from Rr = P(1 + r): w = side_min + pick(Rr0, side_max - side_min + 1), h likewise from Rr1; the
// centre (cx, cy) = (pick(Rr2, S), pick(Rr3, S)), or with centre == JOINT and nv > 0 the pixel of the pick(Rr2, nv)-th
// joint, in index order, among the nv joints with mask != 0 whose pixel lies in the image; x0 = max(cx - w/2, 0),
// x1 = min(cx - w/2 + w, S) (integer division), y alike.  Rows count..K-1 of rects are zero.  A joint's pixel is
// (int)floorf((c + 1.f) * (0.5f * S)) per coordinate; NaN or outside [0, S): the joint has no pixel.
// draw == 0: rects and donor are read; every coordinate is clamped into [0, S] and the donor into [0, B), so nothing a
// device tensor holds addresses outside the batch; x1 <= x0 or y1 <= y0 is an empty rectangle.
//
// Fills (where rectangles overlap all of them give the same value): VALUE, channel c = fill_value[c]; NOISE,
// Nw = P(9), ns = Nw0 | Nw1 << 32, the words of pixel q = y S + x are Philox4x32-10 with key ns and counter (q, step lo,
// step hi, DSNT_OCCLUDE_DOMAIN + 10), u = (float)(u24(word c) + 1) * 2^-24 (exact), value = (u - mean[c]) / stdv[c], the
// expression augment_kernel normalises with (built with -ffp-contract=off, build.py); PASTE, the pixel of sample donor
// at the same position of `in`.
//
// Threads: one per OCC_PX = 4 consecutive pixels of a row, all three planes; grid (ceil(ceil(S S / 4) / 256), B).  VEC (S
// a multiple of 4, both tensors 16-byte aligned): a group is one 16-byte load and store per plane, and a group no
// rectangle meets moves its bits untouched (NaN payloads, infinities and -0 included); the rectangle test in front of
// the store is count <= 8 integer compares against LDS broadcasts.  Otherwise a thread moves its pixels one by one (a
// group may then wrap a row).  Thread j < J of every workgroup computes joint j's pixel into LDS, thread 0 derives the
// sample's rectangles from them, as augment_kernel does with its parameters; workgroup 0 of the sample alone writes
// rects, donor and occluded[b][j] = joint j's pixel lies in some rectangle (whatever its mask).
#include "common.h"
#include "philox.h"

namespace {

constexpr int OCC_NT = 256;
constexpr int OCC_PX = 4;
static_assert(DSNT_OCCLUDE_MAX_JOINTS <= OCC_NT, "one thread per joint");

struct OccArgs {
    const uint32_t* in;         // the bit patterns: nothing outside a rectangle goes through a float operation
    uint32_t* out;
    const float *fill_value, *mean, *stdv, *coords, *mask;
    int32_t *rects, *donor;
    uint8_t* occluded;
    uint64_t seed, step;
    uint32_t draw_offset, p24;
    int B, S, K, J, side_min, side_span, fill, centre, draw;
};

struct OccSample {
    int x0[DSNT_OCCLUDE_MAX_RECTS], y0[DSNT_OCCLUDE_MAX_RECTS], x1[DSNT_OCCLUDE_MAX_RECTS], y1[DSNT_OCCLUDE_MAX_RECTS];
    int count, donor;
    uint64_t ns;
    float fv[3], mean[3], std[3];
};

__device__ __forceinline__ uint32_t pick(uint32_t x, int n) { return (uint32_t)(((uint64_t)(x >> 8) * (uint64_t)n) >> 24); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Thread 0: the sample's rectangles, donor and noise key into LDS.  jx, jy: the joints' pixels (-1: none); jc: 1 where the
// joint may centre a rectangle.
__device__ void occ_sample(const OccArgs& a, int b, OccSample& s, const int* jx, const int* jy, const uint8_t* jc) {
    const uint32_t g = a.draw_offset + (uint32_t)b;
    const int S = a.S, K = a.K;
    uint32_t w[4];
    Philox::gen(w, a.seed, a.step, g, DSNT_OCCLUDE_DOMAIN + 9u);
    s.ns = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    for (int c = 0; c < 3; ++c) {
        s.fv[c] = a.fill_value[c];
        s.mean[c] = a.mean[c];
        s.std[c] = a.stdv[c];
    }
    if (!a.draw) {
        for (int r = 0; r < K; ++r) {
            const int32_t* q = a.rects + ((size_t)b * K + r) * 4;
            s.x0[r] = clampi(q[0], 0, S);
            s.y0[r] = clampi(q[1], 0, S);
            s.x1[r] = clampi(q[2], 0, S);
            s.y1[r] = clampi(q[3], 0, S);
        }
        s.count = K;
        s.donor = clampi(a.donor[b], 0, a.B - 1);
        return;
    }
    Philox::gen(w, a.seed, a.step, g, DSNT_OCCLUDE_DOMAIN);
    const int count = (w[0] >> 8) < a.p24 ? 1 + (int)pick(w[1], K) : 0;
    s.count = count;
    s.donor = a.B > 1 ? (int)(((uint32_t)b + 1u + pick(w[2], a.B - 1)) % (uint32_t)a.B) : b;
    int nv = 0;
    for (int j = 0; j < a.J; ++j) nv += jc[j];
    for (int r = 0; r < K; ++r) {
        int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (r < count) {
            Philox::gen(w, a.seed, a.step, g, DSNT_OCCLUDE_DOMAIN + 1u + (uint32_t)r);
            const int rw = a.side_min + (int)pick(w[0], a.side_span), rh = a.side_min + (int)pick(w[1], a.side_span);
            int cx, cy;
            if (nv > 0) {
                int t = (int)pick(w[2], nv), j = 0;
                for (;; ++j) {                          // the t-th joint with jc != 0: t < nv, so it ends below J
                    if (jc[j] && t-- == 0) break;
                }
                cx = jx[j];
                cy = jy[j];
            } else {
                cx = (int)pick(w[2], S);
                cy = (int)pick(w[3], S);
            }
            x0 = max(cx - rw / 2, 0);
            x1 = min(cx - rw / 2 + rw, S);
            y0 = max(cy - rh / 2, 0);
            y1 = min(cy - rh / 2 + rh, S);
        }
        s.x0[r] = x0; s.y0[r] = y0; s.x1[r] = x1; s.y1[r] = y1;
    }
    if (blockIdx.x == 0) {
        for (int r = 0; r < K; ++r) {
            int32_t* q = a.rects + ((size_t)b * K + r) * 4;
            q[0] = s.x0[r]; q[1] = s.y0[r]; q[2] = s.x1[r]; q[3] = s.y1[r];
        }
        a.donor[b] = s.donor;
    }
}

__device__ __forceinline__ bool occ_inside(const OccSample& s, int x, int y) {
    bool in = false;
    for (int r = 0; r < s.count; ++r) in = in || (x >= s.x0[r] && x < s.x1[r] && y >= s.y0[r] && y < s.y1[r]);
    return in;
}

// The fill of pixel q (= y S + x) of the sample: the three channels' bit patterns.  don: the donor sample of `in`.
__device__ __forceinline__ void occ_fill(const OccArgs& a, const OccSample& s, const uint32_t* __restrict__ don, size_t plane,
                                         int q, uint32_t val[3]) {
    if (a.fill == DSNT_OCCLUDE_FILL_VALUE) {
        for (int c = 0; c < 3; ++c) val[c] = __float_as_uint(s.fv[c]);
    } else if (a.fill == DSNT_OCCLUDE_FILL_NOISE) {
        uint32_t o[4];
        Philox::gen(o, s.ns, a.step, (uint32_t)q, DSNT_OCCLUDE_DOMAIN + 10u);
        for (int c = 0; c < 3; ++c) {
            const float u = (float)((o[c] >> 8) + 1u) * (1.f / 16777216.f);
            val[c] = __float_as_uint((u - s.mean[c]) / s.std[c]);
        }
    } else {
        for (int c = 0; c < 3; ++c) val[c] = don[c * plane + q];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(OCC_NT) occlude_kernel(const OccArgs a) {
    __shared__ OccSample s;
    __shared__ int jx[DSNT_OCCLUDE_MAX_JOINTS], jy[DSNT_OCCLUDE_MAX_JOINTS];
    __shared__ uint8_t jc[DSNT_OCCLUDE_MAX_JOINTS];
    const int b = blockIdx.y, S = a.S, tid = threadIdx.x;
    if (tid < a.J) {
        const size_t i = (size_t)b * a.J + tid;
        const float half = 0.5f * (float)S;
        const float fx = floorf((a.coords[2 * i] + 1.f) * half), fy = floorf((a.coords[2 * i + 1] + 1.f) * half);
        const bool in = fx >= 0.f && fx < (float)S && fy >= 0.f && fy < (float)S;      // false at NaN
        jx[tid] = in ? (int)fx : -1;
        jy[tid] = in ? (int)fy : -1;
        jc[tid] = in && a.centre == DSNT_OCCLUDE_CENTRE_JOINT && a.mask[i] != 0.f;
    }
    __syncthreads();
    if (tid == 0) occ_sample(a, b, s, jx, jy, jc);
    __syncthreads();
    if (blockIdx.x == 0 && tid < a.J)
        a.occluded[(size_t)b * a.J + tid] = jx[tid] >= 0 && occ_inside(s, jx[tid], jy[tid]) ? 1 : 0;
    const int npx = S * S;                                     // <= 2^24
    const int p0 = (blockIdx.x * OCC_NT + tid) * OCC_PX;
    if (p0 >= npx) return;
    const size_t plane = (size_t)npx;
    const uint32_t* __restrict__ src = a.in + (size_t)b * 3 * plane;
    const uint32_t* __restrict__ don = a.in + (size_t)s.donor * 3 * plane;
    uint32_t* __restrict__ dst = a.out + (size_t)b * 3 * plane;
    if constexpr (VEC) {                                       // S % 4 == 0: the group lies in one row
        const int y = p0 / S, x = p0 - y * S;
        uint4 v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const uint4*>(src + c * plane + p0);
        unsigned hit = 0u;                                     // bit k: pixel x + k lies in some rectangle
        for (int r = 0; r < s.count; ++r) {
            if (y >= s.y0[r] && y < s.y1[r]) {
                const int x0 = s.x0[r], x1 = s.x1[r];
#pragma unroll
                for (int k = 0; k < OCC_PX; ++k) hit |= (x + k >= x0 && x + k < x1) ? 1u << k : 0u;
            }
        }
        if (hit) {
            uint32_t e[3][OCC_PX];
#pragma unroll
            for (int c = 0; c < 3; ++c) { e[c][0] = v[c].x; e[c][1] = v[c].y; e[c][2] = v[c].z; e[c][3] = v[c].w; }
#pragma unroll
            for (int k = 0; k < OCC_PX; ++k) {
                if (hit >> k & 1u) {
                    uint32_t val[3];
                    occ_fill(a, s, don, plane, p0 + k, val);
#pragma unroll
                    for (int c = 0; c < 3; ++c) e[c][k] = val[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = make_uint4(e[c][0], e[c][1], e[c][2], e[c][3]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint4*>(dst + c * plane + p0) = v[c];
    } else {
        for (int k = 0; k < OCC_PX && p0 + k < npx; ++k) {
            const int q = p0 + k, y = q / S, x = q - y * S;
            uint32_t val[3];
            if (occ_inside(s, x, y)) {
                occ_fill(a, s, don, plane, q, val);
            } else {
                for (int c = 0; c < 3; ++c) val[c] = src[c * plane + q];
            }
            for (int c = 0; c < 3; ++c) dst[c * plane + q] = val[c];
        }
    }
}

}  // namespace

extern "C" int dsnt_occlude(const float* in, float* out, int B, int S, int K, int side_min, int side_max, uint32_t p24,
                            int fill, int centre, const float* fill_value, const float* mean, const float* stdv,
                            const float* coords, const float* mask, int J, int32_t* rects, int32_t* donor,
                            uint8_t* occluded, int draw, uint64_t seed, uint64_t step, uint32_t draw_offset,
                            void* stream) {
    DSNT_REQUIRE(in && out && fill_value && mean && stdv && rects && donor, DSNT_ERR_ARG, "dsnt_occlude: null pointer");
    DSNT_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096 && K >= 1 && K <= DSNT_OCCLUDE_MAX_RECTS && J >= 0 &&
                 J <= DSNT_OCCLUDE_MAX_JOINTS, DSNT_ERR_SHAPE, "dsnt_occlude: bad shape B=%d S=%d K=%d J=%d", B, S, K, J);
    DSNT_REQUIRE(side_min >= 1 && side_min <= side_max && side_max <= S, DSNT_ERR_SHAPE,
                 "dsnt_occlude: sides %d..%d outside 1 <= side_min <= side_max <= S=%d", side_min, side_max, S);
    DSNT_REQUIRE(fill == DSNT_OCCLUDE_FILL_VALUE || fill == DSNT_OCCLUDE_FILL_NOISE || fill == DSNT_OCCLUDE_FILL_PASTE,
                 DSNT_ERR_ARG, "dsnt_occlude: unknown fill %d", fill);
    DSNT_REQUIRE(centre == DSNT_OCCLUDE_CENTRE_UNIFORM || centre == DSNT_OCCLUDE_CENTRE_JOINT, DSNT_ERR_ARG,
                 "dsnt_occlude: unknown centre %d", centre);
    DSNT_REQUIRE(p24 <= (1u << 24), DSNT_ERR_ARG, "dsnt_occlude: p24=%u above 2^24", p24);
    DSNT_REQUIRE(J == 0 || (coords && occluded && (mask || centre != DSNT_OCCLUDE_CENTRE_JOINT)), DSNT_ERR_ARG,
                 "dsnt_occlude: J=%d joints need coords and occluded, and joint centring a mask", J);
    const uintptr_t bytes = (uintptr_t)B * 3u * (uintptr_t)S * (uintptr_t)S * sizeof(float);
    const uintptr_t pi = (uintptr_t)in, po = (uintptr_t)out;
    DSNT_REQUIRE(pi != po && (pi < po ? po - pi >= bytes : pi - po >= bytes), DSNT_ERR_ARG,
                 "dsnt_occlude: in and out overlap (the kernel is out of place: the paste fill reads other samples of in)");
    OccArgs a;
    a.in = (const uint32_t*)in;
    a.out = (uint32_t*)out;
    a.fill_value = fill_value; a.mean = mean; a.stdv = stdv; a.coords = coords; a.mask = mask;
    a.rects = rects; a.donor = donor; a.occluded = occluded;
    a.seed = seed; a.step = step; a.draw_offset = draw_offset; a.p24 = p24;
    a.B = B; a.S = S; a.K = K; a.J = J; a.side_min = side_min; a.side_span = side_max - side_min + 1;
    a.fill = fill; a.centre = centre; a.draw = draw != 0;
    const int groups = (S * S + OCC_PX - 1) / OCC_PX;
    const dim3 grid((groups + OCC_NT - 1) / OCC_NT, B);
    if (S % OCC_PX == 0 && dsnt_aligned16(in) && dsnt_aligned16(out))
        DSNT_LAUNCH(occlude_kernel<true>, grid, dim3(OCC_NT), 0, (hipStream_t)stream, a);
    else
        DSNT_LAUNCH(occlude_kernel<false>, grid, dim3(OCC_NT), 0, (hipStream_t)stream, a);
    DSNT_CHECK_LAUNCH("dsnt_occlude");
}
