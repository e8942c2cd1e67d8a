// Per-step operand preparation of the convolution kernels: tensor maxima (the fp16x3 operand bounds), the bf16 / fp16 plane
// splits of weights (plain, stream and space-to-depth layouts), the BatchNorm operand bounds and the data-gradient weight packs.
#include "conv_split.h"

__global__ void split_bf16x3_kernel(const float4* __restrict__ src, uint2* __restrict__ dst, long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        uint2 a, b, c;
        split4(src[i], a, b, c);
        dst[i] = a; dst[n4 + i] = b; dst[2 * n4 + i] = c;
    }
}

extern "C" int dsnt_split_bf16x3(const float* src, void* dst, int64_t n, void* stream) {
    DSNT_REQUIRE(src && dst && n > 0 && n % 4 == 0, DSNT_ERR_ARG, "dsnt_split_bf16x3: n must be a positive multiple of 4");
    DSNT_REQUIRE(dsnt_aligned16(src) && (((uintptr_t)dst) & 7u) == 0, DSNT_ERR_ALIGN, "dsnt_split_bf16x3: alignment");
    const long n4 = n / 4;
    long g = (n4 + 255) / 256;
    if (g > 2048) g = 2048;
    DSNT_LAUNCH(split_bf16x3_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)src, (uint2*)dst, n4);
    DSNT_CHECK_LAUNCH("dsnt_split_bf16x3");
}

// max |src[i]| -> out[0] (bit pattern of a non-negative float: integer max is float max)
__global__ void amax_kernel(const float4* __restrict__ src, unsigned* __restrict__ out, long n4) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = src[i];
        m = fmaxf(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))), m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out + (blockIdx.x & (DSNT_BOUND_SLOTS - 1)), __float_as_uint(m));
}

extern "C" int dsnt_amax(const float* src, int64_t n, float* out, void* stream) {
    DSNT_REQUIRE(src && out && n > 0 && n % 4 == 0 && dsnt_aligned16(src), DSNT_ERR_ARG,
                 "dsnt_amax: n must be a positive multiple of 4, src 16-byte aligned");
    DSNT_REQUIRE(!dsnt_recording(), DSNT_ERR_ARG, "dsnt_amax: cannot be recorded into a launch list (it clears its output with a memset)");
    if (hipMemsetAsync(out, 0, 4 * DSNT_BOUND_SLOTS, (hipStream_t)stream) != hipSuccess) return dsnt_set_error(DSNT_ERR_HIP, "dsnt_amax: memset");
    long g = (n / 4 + 255) / 256;
    if (g > 1024) g = 1024;
    DSNT_LAUNCH(amax_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const float4*)src,
                       (unsigned*)out, (long)(n / 4));
    DSNT_CHECK_LAUNCH("dsnt_amax");
}

__global__ void split_f16x2_kernel(const float4* __restrict__ src, uint2* __restrict__ dst, long n4, long stride4,
                                   const float* __restrict__ bound) {
    const float sc = pow2_scale(bound64(bound));
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 v = src[i];
        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        uint2 a, b;
        split4h(v, a, b);
        dst[i] = a; dst[stride4 + i] = b;
    }
}

extern "C" int dsnt_split_f16x2(const float* src, void* dst, int64_t n, int64_t plane_stride, const float* bound,
                                void* stream) {
    DSNT_REQUIRE(src && dst && bound && n > 0 && n % 4 == 0 && plane_stride >= n && plane_stride % 4 == 0, DSNT_ERR_ARG,
                 "dsnt_split_f16x2: n and plane_stride must be positive multiples of 4, plane_stride >= n");
    DSNT_REQUIRE(dsnt_aligned16(src) && (((uintptr_t)dst) & 7u) == 0, DSNT_ERR_ALIGN, "dsnt_split_f16x2: alignment");
    const long n4 = n / 4;
    long g = (n4 + 255) / 256;
    if (g > 2048) g = 2048;
    DSNT_LAUNCH(split_f16x2_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const float4*)src,
                       (uint2*)dst, n4, (long)(plane_stride / 4), bound);
    DSNT_CHECK_LAUNCH("dsnt_split_f16x2");
}

// Per-step preparation of the fp16x3 operands of MANY tensors in one launch each (table rows of int64):
//   dsnt_f16_prep_weights: row {src float*, dst fp16 plane 0*, bound float*, count (multiple of 4), plane stride,
//     stream Cout, stream Cin}: one workgroup per row: bound = max|src|, then dst = two fp16 planes of src * pow2_scale(bound);
//     stream Cout > 0: src is an OHWI 3x3 filter [Cout][3][3][Cin] and the planes are written in STREAM order
//     [Cin / 16][9 taps][Cout][16] — the K-step sequence of conv3s.hip, each step one contiguous block;
//   dsnt_f16_prep_bn_bounds: row {gamma float*, beta float*, out float*, C, float bits of sqrt(M)}: out =
//     max_c(|gamma_c| sqrt(M) + |beta_c|) >= every |relu?(bn(x))| of a train-mode BatchNorm over M samples
//     (|(x - mean) / std| <= sqrt(M - 1) for the biased batch variance).
// (1024 threads and four independent loads per thread and pass: one workgroup walks a whole tensor, so the launch lasts as
// long as its largest row — 130 us for a 3x3 128->128 filter with 256 threads and one load in flight, and proportionally longer
// on hg8, where the stem convolution no longer covers it.)
#define PREP_T 1024
__global__ __launch_bounds__(PREP_T) void f16_prep_weights_kernel(const long long* __restrict__ table, int row_ints) {
    __shared__ float red[PREP_T / 64];
    const long long* t = table + (size_t)blockIdx.x * row_ints;
    const float4* src = reinterpret_cast<const float4*>(t[0]);
    uint2* dst = reinterpret_cast<uint2*>(t[1]);
    float* bound = reinterpret_cast<float*>(t[2]);
    const long n4 = (long)t[3] / 4, stride4 = (long)t[4] / 4;
    // > 0: OHWI [Cout][9][Cin] -> stream order [Cin/16][9][Cout][16] (rows of 5 values: always the plain layout)
    const int s_cout = row_ints >= 7 ? (int)t[5] : 0, s_cin = row_ints >= 7 ? (int)t[6] : 0;
    const int s_k4 = 9 * s_cin / 4, s_cin4 = s_cin / 4;
    float m = 0.f;
    long i = threadIdx.x;
    for (; i + 3 * PREP_T < n4; i += 4 * PREP_T) {
        const float4 v0 = src[i], v1 = src[i + PREP_T], v2 = src[i + 2 * PREP_T], v3 = src[i + 3 * PREP_T];
        m = fmaxf(fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w))), m);
        m = fmaxf(fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w))), m);
        m = fmaxf(fmaxf(fmaxf(fabsf(v2.x), fabsf(v2.y)), fmaxf(fabsf(v2.z), fabsf(v2.w))), m);
        m = fmaxf(fmaxf(fmaxf(fabsf(v3.x), fabsf(v3.y)), fmaxf(fabsf(v3.z), fabsf(v3.w))), m);
    }
    for (; i < n4; i += PREP_T) {
        const float4 v = src[i];
        m = fmaxf(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))), m);
    }
    m = block_max(m, red);
    if (threadIdx.x < DSNT_BOUND_SLOTS) bound[threadIdx.x] = m;
    const float sc = pow2_scale(m);
    auto put = [&](long j, float4 v) {
        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        uint2 a, b;
        split4h(v, a, b);
        if (s_cout > 0) {
            const int n = (int)(j / s_k4), k4 = (int)(j - (long)n * s_k4);
            const int tap = k4 / s_cin4, c4 = k4 - tap * s_cin4;
            j = ((long)((c4 >> 2) * 9 + tap) * s_cout + n) * 4 + (c4 & 3);
        }
        dst[j] = a; dst[stride4 + j] = b;
    };
    i = threadIdx.x;
    for (; i + 3 * PREP_T < n4; i += 4 * PREP_T) {
        const float4 v0 = src[i], v1 = src[i + PREP_T], v2 = src[i + 2 * PREP_T], v3 = src[i + 3 * PREP_T];
        put(i, v0); put(i + PREP_T, v1); put(i + 2 * PREP_T, v2); put(i + 3 * PREP_T, v3);
    }
    for (; i < n4; i += PREP_T) put(i, src[i]);
}

// (the table's row width is an argument: the first form of this entry point read five values per row, and a caller's
// five-wide table must not be walked with a stride of seven)
extern "C" int dsnt_f16_prep_weights(const int64_t* table, int rows, int row_ints, void* stream) {
    DSNT_REQUIRE(table && rows > 0 && (row_ints == 5 || row_ints == 7), DSNT_ERR_ARG,
                 "dsnt_f16_prep_weights: bad argument (row_ints is 5: plain layout only, or 7: with the stream-layout columns)");
    DSNT_LAUNCH(f16_prep_weights_kernel, dim3(rows), dim3(PREP_T), 0, (hipStream_t)stream, (const long long*)table, row_ints);
    DSNT_CHECK_LAUNCH("dsnt_f16_prep_weights");
}

// The stem's per-step weight preparation in ONE small launch (one 256-thread workgroup; 16 K values): the [Cout][4][4][16]
// space-to-depth form of the OHWI [Cout][7][7][4] filter (dsnt_s2d_weights, back = 0), its maximum, and its fp16 (two) and
// bf16 (three) planes — instead of three launches, one of them a 1024-thread workgroup that waits for a free CU at the head of
// every step.
__global__ __launch_bounds__(256) void s2d_weights_prep_kernel(const float* __restrict__ w, float* __restrict__ w2,
                                                               uint2* __restrict__ p16, uint2* __restrict__ p6,
                                                               float* __restrict__ bound, int Cout) {
    __shared__ float red[4];
    const int n4 = Cout * 64;                     // float4 groups of w2: [Cout][4][4][4 blocks-of-4]
    auto fetch = [&](int q) {                     // group q = ((co*4 + R)*4 + S)*4 + (dy*2+dx): four channels of one tap
        const int d = q & 3, S = (q >> 2) & 3, R = (q >> 4) & 3, co = q >> 6;
        const int r = 2 * R + (d >> 1) - 1, s_ = 2 * S + (d & 1) - 1;
        return (r >= 0 && s_ >= 0) ? *reinterpret_cast<const float4*>(w + ((co * 7 + r) * 7 + s_) * 4)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    float m = 0.f;
    auto emit = [&](const int q, const float4 v, const float sc) {
        if (w2) reinterpret_cast<float4*>(w2)[q] = v;
        uint2 a, b, c;
        split4(v, a, b, c);
        p6[q] = a; p6[n4 + q] = b; p6[2 * n4 + q] = c;
        split4h(make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc), a, b);
        p16[q] = a; p16[n4 + q] = b;
    };
    if (n4 <= 16 * 256) {
        // (Cout <= 64, every stem: the 16 groups of a thread are fetched at once and kept — this one-workgroup launch sits on the
        // dependency chain at the head of every step, and 2 x 16 dependent round trips to L2 were 24-55 us of it)
        float4 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int q = threadIdx.x + 256 * j;
            v[j] = q < n4 ? fetch(q) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            m = fmaxf(fmaxf(fmaxf(fabsf(v[j].x), fabsf(v[j].y)), fmaxf(fabsf(v[j].z), fabsf(v[j].w))), m);
        m = block_max(m, red);
        if (threadIdx.x < DSNT_BOUND_SLOTS) bound[threadIdx.x] = m;
        const float sc = pow2_scale(m);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int q = threadIdx.x + 256 * j;
            if (q < n4) emit(q, v[j], sc);
        }
        return;
    }
    for (int q = threadIdx.x; q < n4; q += 256) {
        const float4 v = fetch(q);
        m = fmaxf(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))), m);
    }
    m = block_max(m, red);
    if (threadIdx.x < DSNT_BOUND_SLOTS) bound[threadIdx.x] = m;
    const float sc = pow2_scale(m);
    for (int q = threadIdx.x; q < n4; q += 256) emit(q, fetch(q), sc);
}

extern "C" int dsnt_s2d_weights_prep(const float* w, float* w2, void* planes16, void* planes_bf16, float* bound, int Cout,
                                     void* stream) {
    DSNT_REQUIRE(w && planes16 && planes_bf16 && bound && Cout > 0, DSNT_ERR_ARG, "dsnt_s2d_weights_prep: bad argument");
    DSNT_REQUIRE(dsnt_aligned16(w) && (!w2 || dsnt_aligned16(w2)) && (((uintptr_t)planes16) & 7u) == 0 &&
                 (((uintptr_t)planes_bf16) & 7u) == 0, DSNT_ERR_ALIGN, "dsnt_s2d_weights_prep: alignment");
    DSNT_LAUNCH(s2d_weights_prep_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, w, w2, (uint2*)planes16, (uint2*)planes_bf16,
                bound, Cout);
    DSNT_CHECK_LAUNCH("dsnt_s2d_weights_prep");
}

__global__ __launch_bounds__(64) void f16_prep_bn_bounds_kernel(const long long* __restrict__ table) {
    const long long* t = table + (size_t)blockIdx.x * 5;
    const float* gamma = reinterpret_cast<const float*>(t[0]);
    const float* beta = reinterpret_cast<const float*>(t[1]);
    float* out = reinterpret_cast<float*>(t[2]);
    const int C = (int)t[3];
    const float sqrtM = __uint_as_float((unsigned)t[4]);
    float m = 0.f;
    for (int c = threadIdx.x; c < C; c += 64) m = fmaxf(m, fmaf(fabsf(gamma[c]), sqrtM, fabsf(beta[c])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    out[threadIdx.x] = m;                    // all DSNT_BOUND_SLOTS entries
}

extern "C" int dsnt_f16_prep_bn_bounds(const int64_t* table, int rows, void* stream) {
    DSNT_REQUIRE(table && rows > 0, DSNT_ERR_ARG, "dsnt_f16_prep_bn_bounds: bad argument");
    DSNT_LAUNCH(f16_prep_bn_bounds_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, (const long long*)table);
    DSNT_CHECK_LAUNCH("dsnt_f16_prep_bn_bounds");
}

// wd[ci][R-1-r][S-1-s][co] = w[co][r][s][ci]
__global__ void pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wd, int Cout,
                                  int R, int S, int Cin) {
    const int total = Cout * R * S * Cin;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int co = i % Cout;
        int t = i / Cout;
        const int s = t % S; t /= S;
        const int r = t % R;
        const int ci = t / R;
        wd[i] = w[((co * R + (R - 1 - r)) * S + (S - 1 - s)) * Cin + ci];
    }
}

extern "C" int dsnt_conv_pack_dgrad(const float* w, float* wd, int Cout, int R, int S, int Cin,
                                    void* stream) {
    DSNT_REQUIRE(w && wd && Cout > 0 && R > 0 && S > 0 && Cin > 0, DSNT_ERR_ARG,
                 "dsnt_conv_pack_dgrad: bad argument");
    const int total = Cout * R * S * Cin;
    const int grid = (total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024;
    DSNT_LAUNCH(pack_dgrad_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, wd, Cout,
                       R, S, Cin);
    DSNT_CHECK_LAUNCH("dsnt_conv_pack_dgrad");
}

// All data-gradient weight packs of a backward pass in ONE launch: for conv c (table row c =
// {src offset, dst offset, Cout, R, S, Cin}) write wd[ci][R-1-r][S-1-s][co] = w[co][r][s][ci] as fp32
// and as three bf16 planes (plane stride = `total` elements).
// One tap of one convolution is a [Cout][Cin] matrix with row pitch R S Cin; it lands transposed, [Cin][Cout] with row pitch
// R S Cout.  32 x 32 tiles through LDS: 128-byte runs along ci on the way in, along co on the way out (element by element the
// reads were 4 bytes per cache line: 360 MB fetched for the 27 MB of hg2's weights, and — 24 000 workgroups for hg8 — a flood that
// kept the dependency chain's 4-workgroup BatchNorm finalise waiting 140-240 us for a slot at the start of every step).
__global__ __launch_bounds__(256) void pack_dgrad_all_kernel(const int* __restrict__ table, const float* __restrict__ params,
                                                            float* __restrict__ out, unsigned short* __restrict__ planes, long total) {
    __shared__ float tl[32][33];
    const int* t = table + blockIdx.y * 6;
    const int src = t[0], dst = t[1], Cout = t[2], R = t[3], S = t[4], Cin = t[5];
    const float* w = params + src;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int cits = (Cin + 31) >> 5, cots = (Cout + 31) >> 5, RS = R * S;
    const int ntiles = RS * cits * cots;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tap = tile % RS;
        int q = tile / RS;
        const int cit = q % cits, cot = q / cits;
        const int r = tap / S, s_ = tap - r * S;            // DESTINATION tap; the source is the flipped one
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = cot * 32 + ty + 8 * i, ci = cit * 32 + tx;
            tl[ty + 8 * i][tx] = (co < Cout && ci < Cin) ? w[((co * R + (R - 1 - r)) * S + (S - 1 - s_)) * Cin + ci] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ci = cit * 32 + ty + 8 * i, co = cot * 32 + tx;
            if (ci < Cin && co < Cout) {
                const float v = tl[tx][ty + 8 * i];
                const long o = (long)dst + ((long)(ci * R + r) * S + s_) * Cout + co;
                out[o] = v;
                // exact 3-way bf16 split (round-to-nearest-even by hand: one scalar at a time)
                float rem = v;
                for (int pl = 0; pl < 3; ++pl) {
                    unsigned u = __float_as_uint(rem);
                    unsigned rb = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
                    planes[(long)pl * total + o] = (unsigned short)(rb >> 16);
                    rem -= __uint_as_float(rb);
                }
            }
        }
        __syncthreads();
    }
}

extern "C" int dsnt_conv_pack_dgrad_all(const int* table, int nconv, const float* params, float* out,
                                        void* planes, int64_t total, void* stream) {
    DSNT_REQUIRE(table && params && out && planes && nconv > 0 && total > 0, DSNT_ERR_ARG,
                 "dsnt_conv_pack_dgrad_all: bad argument");
    DSNT_LAUNCH(pack_dgrad_all_kernel, dim3(16, nconv), dim3(256), 0, (hipStream_t)stream, table, params,
                       out, (unsigned short*)planes, (long)total);
    DSNT_CHECK_LAUNCH("dsnt_conv_pack_dgrad_all");
}
