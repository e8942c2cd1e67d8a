// BatchNorm on NHWC: the per-channel tile reductions and their fp64 finalisation (deterministic, no atomics), the
// scale/shift + ReLU apply forward (plain, with a residual, with the output's statistics) and its backward.  Stands for
// nn.BatchNorm2d + relu of the reference's residual blocks (hourglass.py:19-24) and torchvision's block tail.
// All 16-byte vectorised (C % 4 == 0).
#include "common.h"
#include <string.h>
#include "bn_pro.h"
#include "ew_bodies.h"

// ---------------------------------------------------------------- per-channel tile reductions
// MODE 0: (sum x, sum x^2)          MODE 1: (sum dz, sum dz*xhat) for y = relu?(bn(x))
// MODE 2: the same sums for y = relu?(bn(x) + skip) (the tail of a torchvision residual block): the ReLU mask comes from the stored
// output (`ymask` > 0) and dz = a * mask is WRITTEN (`dz_out`: the skip branch's gradient and the apply pass read it)
template <int MODE>
__global__ __launch_bounds__(256) void tile_reduce_kernel(
    const float* __restrict__ a, const float* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, int relu, float* __restrict__ partial, long M, int C, int cgs,
    const float* __restrict__ ymask = nullptr, float* __restrict__ dz_out = nullptr) {
    __shared__ float red[256 * 8];
    const int tid = threadIdx.x;
    const int C4 = C >> 2;
    const int rpar = 256 / cgs;               // row lanes (cgs = column groups handled per pass: tile_cgs)
    const int cg_l = tid % cgs, rl = tid / cgs;
    const bool active = rl < rpar;
    const long row0 = (long)blockIdx.x * TILE_ROWS;
    const long row1 = row0 + TILE_ROWS < M ? row0 + TILE_ROWS : M;
    for (int cg0 = blockIdx.y * cgs; cg0 < C4; cg0 += cgs * gridDim.y) {
        const int cg = cg0 + cg_l;
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
        if (active && cg < C4) {
            float4 sc, sh, mu, is;
            if (MODE == 1) {
                sc = reinterpret_cast<const float4*>(scale)[cg];
                sh = reinterpret_cast<const float4*>(shift)[cg];
            }
            if (MODE >= 1) {
                mu = reinterpret_cast<const float4*>(mean)[cg];
                is = reinterpret_cast<const float4*>(invstd)[cg];
            }
            for (long r = row0 + rl; r < row1; r += rpar) {
                const float4 v = reinterpret_cast<const float4*>(a + r * C)[cg];
                if (MODE == 0) {
                    s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
                    s2.x = fmaf(v.x, v.x, s2.x); s2.y = fmaf(v.y, v.y, s2.y);
                    s2.z = fmaf(v.z, v.z, s2.z); s2.w = fmaf(v.w, v.w, s2.w);
                } else {
                    const float4 xv = reinterpret_cast<const float4*>(x + r * C)[cg];
                    float4 dz = v;
                    if (MODE == 2) {
                        if (relu) {
                            const float4 yv = reinterpret_cast<const float4*>(ymask + r * C)[cg];
                            if (yv.x <= 0.f) dz.x = 0.f;
                            if (yv.y <= 0.f) dz.y = 0.f;
                            if (yv.z <= 0.f) dz.z = 0.f;
                            if (yv.w <= 0.f) dz.w = 0.f;
                        }
                        reinterpret_cast<float4*>(dz_out + r * C)[cg] = dz;
                    } else if (relu) {
                        if (fmaf(xv.x, sc.x, sh.x) <= 0.f) dz.x = 0.f;
                        if (fmaf(xv.y, sc.y, sh.y) <= 0.f) dz.y = 0.f;
                        if (fmaf(xv.z, sc.z, sh.z) <= 0.f) dz.z = 0.f;
                        if (fmaf(xv.w, sc.w, sh.w) <= 0.f) dz.w = 0.f;
                    }
                    s1.x += dz.x; s1.y += dz.y; s1.z += dz.z; s1.w += dz.w;
                    s2.x = fmaf(dz.x, (xv.x - mu.x) * is.x, s2.x);
                    s2.y = fmaf(dz.y, (xv.y - mu.y) * is.y, s2.y);
                    s2.z = fmaf(dz.z, (xv.z - mu.z) * is.z, s2.z);
                    s2.w = fmaf(dz.w, (xv.w - mu.w) * is.w, s2.w);
                }
            }
        }
        __syncthreads();
        float* mine = red + tid * 8;
        mine[0] = s1.x; mine[1] = s1.y; mine[2] = s1.z; mine[3] = s1.w;
        mine[4] = s2.x; mine[5] = s2.y; mine[6] = s2.z; mine[7] = s2.w;
        __syncthreads();
        if (tid < cgs && cg0 + tid < C4) {
            float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < rpar; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += red[(j * cgs + tid) * 8 + e];
            float* p0 = partial + ((size_t)blockIdx.x * 2 + 0) * C + (size_t)(cg0 + tid) * 4;
            float* p1 = partial + ((size_t)blockIdx.x * 2 + 1) * C + (size_t)(cg0 + tid) * 4;
            *reinterpret_cast<float4*>(p0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            *reinterpret_cast<float4*>(p1) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        }
    }
}

extern "C" int dsnt_bn_stats(const float* x, float* partial, int64_t M, int C, void* stream) {
    DSNT_REQUIRE(x && partial && M > 0 && C > 0, DSNT_ERR_ARG, "dsnt_bn_stats: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(partial), DSNT_ERR_ALIGN,
                 "dsnt_bn_stats: C %% 4 and 16-byte alignment required");
    const int tiles = (int)((M + TILE_ROWS - 1) / TILE_ROWS);
    DSNT_LAUNCH(tile_reduce_kernel<0>, dim3(tiles, tile_grid_y(tiles, C / 4)), dim3(256), 0, (hipStream_t)stream, x,
                       nullptr, nullptr, nullptr, nullptr, nullptr, 0, partial, (long)M, C, tile_cgs(tiles, C / 4));
    DSNT_CHECK_LAUNCH("dsnt_bn_stats");
}

// OP 2 of tile_op_stats_kernel (resample.hip describes the family): y = relu?(a * bn_scale + bn_shift) with the BatchNorm
// statistics of y in the same pass (the stem's materialised BatchNorm + ReLU, hourglass.py:157-159).
extern "C" int dsnt_bn_act_fwd_stats(const float* x, const float* scale, const float* shift, int relu, float* y,
                                     float* partial, int64_t M, int C, const dsnt_out_bounds* g_tail, void* stream) {
    OutBoundsP tail;
    if (int e = out_bounds_fill(tail, g_tail, "dsnt_bn_act_fwd_stats")) return e;
    DSNT_REQUIRE(x && scale && shift && y && M > 0 && C > 0, DSNT_ERR_ARG, "dsnt_bn_act_fwd_stats: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(y) && dsnt_aligned16(scale) && dsnt_aligned16(shift) &&
                 dsnt_aligned16(partial), DSNT_ERR_ALIGN, "dsnt_bn_act_fwd_stats: alignment");
    const long tiles = ((long)M + TILE_ROWS - 1) / TILE_ROWS;
    // rows are flat here: N = 1, Ho = 1, Wo = M would overflow int for nothing — the kernel only needs M = N*Ho*Wo
    DSNT_REQUIRE(M < (1ll << 31), DSNT_ERR_SHAPE, "dsnt_bn_act_fwd_stats: M too large");
    const TileOpP q{x, nullptr, y, nullptr, partial, 1, 1, (int)M, C, tile_cgs(tiles, C / 4), tail, scale, shift, relu};
    DSNT_LAUNCH(tile_op_stats_kernel<2>, dim3((unsigned)tiles, tile_grid_y(tiles, C / 4)), dim3(256), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_bn_act_fwd_stats");
}

extern "C" int dsnt_bn_act_bwd_reduce(const float* da, const float* x, const float* scale,
                                      const float* shift, const float* mean, const float* invstd,
                                      int relu, float* partial, int64_t M, int C, void* stream) {
    DSNT_REQUIRE(da && x && scale && shift && mean && invstd && partial && M > 0 && C > 0,
                 DSNT_ERR_ARG, "dsnt_bn_act_bwd_reduce: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(da) && dsnt_aligned16(partial) &&
                 dsnt_aligned16(scale) && dsnt_aligned16(shift) && dsnt_aligned16(mean) &&
                 dsnt_aligned16(invstd), DSNT_ERR_ALIGN,
                 "dsnt_bn_act_bwd_reduce: C %% 4 and 16-byte alignment required");
    const int tiles = (int)((M + TILE_ROWS - 1) / TILE_ROWS);
    DSNT_LAUNCH(tile_reduce_kernel<1>, dim3(tiles, tile_grid_y(tiles, C / 4)), dim3(256), 0, (hipStream_t)stream, da, x,
                       scale, shift, mean, invstd, relu, partial, (long)M, C, tile_cgs(tiles, C / 4));
    DSNT_CHECK_LAUNCH("dsnt_bn_act_bwd_reduce");
}

// The backward of y = relu?(bn(x) + skip) up to the BatchNorm's two reductions, in one pass: dz = da * (y > 0) written, and the
// tile sums (sum dz, sum dz * xhat) for dsnt_bn_bwd_finalize — dsnt_relu_bwd + dsnt_bn_act_bwd_reduce(relu = 0) as one launch.
extern "C" int dsnt_bn_add_act_bwd_reduce(const float* da, const float* y, const float* x, const float* mean, const float* invstd,
                                          int relu, float* dz, float* partial, int64_t M, int C, void* stream) {
    DSNT_REQUIRE(da && y && x && mean && invstd && dz && partial && M > 0 && C > 0, DSNT_ERR_ARG, "dsnt_bn_add_act_bwd_reduce: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(da) && dsnt_aligned16(y) && dsnt_aligned16(dz) && dsnt_aligned16(partial) &&
                 dsnt_aligned16(mean) && dsnt_aligned16(invstd), DSNT_ERR_ALIGN, "dsnt_bn_add_act_bwd_reduce: C %% 4 and 16-byte alignment required");
    const int tiles = (int)((M + TILE_ROWS - 1) / TILE_ROWS);
    DSNT_LAUNCH(tile_reduce_kernel<2>, dim3(tiles, tile_grid_y(tiles, C / 4)), dim3(256), 0, (hipStream_t)stream, da, x,
                       nullptr, nullptr, mean, invstd, relu, partial, (long)M, C, tile_cgs(tiles, C / 4), y, dz);
    DSNT_CHECK_LAUNCH("dsnt_bn_add_act_bwd_reduce");
}

// Combine tile partials: 16 channels x 64 tile-lanes per 1024-thread block (the kernel is pure
// latency: many independent loads in flight matter, not bandwidth), fp64 accumulation.
// MODE 0: forward statistics.  MODE 1: backward sums.
#define FIN_T 1024
#define FIN_P (FIN_T / 16)
// MODE 1, optional: the bound of dx = scale (dz - coef0 - xhat coef1) for a consumer that forms dx in registers
// (dsnt_conv1x1_bwd_f16x3): max_c |scale_c| (max|dz| + |coef0_c| + |coef1_c| sqrt(M)), |xhat| <= sqrt(M) for the batch
// statistics of M samples; raised into the 64 slots of `out` like every other bound
struct BnBoundP { const float* scale; const float* dz_amax; float sqrtM; unsigned* out; };
struct BnFinP {
    const float* partial; int ntiles; double invM, unbias; int C;
    const float* gamma; const float* beta; float* running_mean; float* running_var;
    float momentum, eps; int training; float* o0; float* o1; float* o2; float* o3; int accumulate; BnBoundP bp;
};
// One workgroup per 16 channels.
template <int MODE>
__global__ __launch_bounds__(FIN_T) void bn_finalize_kernel(BnFinP q) {
    __shared__ double r0[256], r1[256];
    const float* __restrict__ partial = q.partial; const int ntiles = q.ntiles; const double invM = q.invM, unbias = q.unbias;
    const int C = q.C; const float* __restrict__ gamma = q.gamma; const float* __restrict__ beta = q.beta;
    float* running_mean = q.running_mean; float* running_var = q.running_var; const float momentum = q.momentum, eps = q.eps;
    const int training = q.training; float* o0 = q.o0; float* o1 = q.o1; float* o2 = q.o2; float* o3 = q.o3;
    const int accumulate = q.accumulate; const BnBoundP bp = q.bp;
    const int tid = threadIdx.x, cl = tid & 15;
    const int wg = blockIdx.x;
    const int c = wg * 16 + cl;
    // everything the last step needs besides the sums is fetched NOW, under the row loop: the kernel's length is what a BatchNorm
    // costs the dependency chain, and a load issued behind the reduction is a microsecond of it (round 5, box N)
    const bool lead = tid < 16 && c < C;
    float pg = 1.f, pb = 0.f, prm = 0.f, prv = 0.f, po0 = 0.f, po1 = 0.f, psc = 0.f, pdz = 0.f;
    if (MODE == 0 && lead) {
        if (gamma) pg = gamma[c];
        if (beta) pb = beta[c];
        if (running_mean) { prm = running_mean[c]; prv = running_var[c]; }
    }
    if (MODE == 1) {
        if (lead && accumulate) { if (o0) po0 = o0[c]; if (o1) po1 = o1[c]; }
        if (bp.out) { pdz = bp.dz_amax[tid & 63]; if (lead) psc = bp.scale[c]; }
    }
    // (VP = 1: the sums as one-element arrays under one-trip loops.  As plain scalars the same row loop compiles to 6 / 16 more
    // instructions and two more SGPRs (MODE 0 / 1); this form is instruction for instruction no larger than before)
    constexpr int VP = 1;
    double a0[VP], a1[VP];
#pragma unroll
    for (int v = 0; v < VP; ++v) {
        a0[v] = 0.0; a1[v] = 0.0;
        const int part = (tid + v * FIN_T) >> 4;
        if (c < C && (MODE == 1 || training)) {
#pragma unroll 4
            for (int t = part; t < ntiles; t += FIN_P) {
                a0[v] += (double)partial[((size_t)t * 2 + 0) * C + c];
                a1[v] += (double)partial[((size_t)t * 2 + 1) * C + c];
            }
        }
    }
    // the four tile-lanes of a wave by shuffles, the waves through LDS, summed by the block's first 16 threads in a fixed order
    // (deterministic; ONE barrier — a seven-level tree over 1024 threads cost the chain ~0.5 us per BatchNorm, round 5)
#pragma unroll
    for (int v = 0; v < VP; ++v) {
        a0[v] += __shfl_xor(a0[v], 16, 64); a1[v] += __shfl_xor(a1[v], 16, 64);
        a0[v] += __shfl_xor(a0[v], 32, 64); a1[v] += __shfl_xor(a1[v], 32, 64);
        if ((tid & 63) < 16) { r0[((tid + v * FIN_T) >> 6) * 16 + cl] = a0[v]; r1[((tid + v * FIN_T) >> 6) * 16 + cl] = a1[v]; }
    }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    if (tid < 16) {
#pragma unroll
        for (int w = 0; w < FIN_T / 64; ++w) { s0 += r0[w * 16 + cl]; s1 += r1[w * 16 + cl]; }
    }
    if (tid < 16 && c < C) {
        if (MODE == 0) {
            double mean, var;
            if (training) {
                mean = s0 * invM;
                var = s1 * invM - mean * mean;
                if (var < 0.0) var = 0.0;
                if (running_mean) {
                    running_mean[c] = (float)((1.0 - momentum) * prm + momentum * mean);
                    running_var[c] = (float)((1.0 - momentum) * prv + momentum * var * unbias);
                }
            } else {
                mean = prm;
                var = prv;
            }
            const float is = (float)(1.0 / sqrt(var + (double)eps));
            const float mu = (float)mean;
            const float sc = gamma ? pg * is : is;
            o0[c] = mu; o1[c] = is; o2[c] = sc;
            o3[c] = (beta ? pb : 0.f) - mu * sc;
        } else {
            // o0 = dgamma, o1 = dbeta, o2 = coef [2][C]
            const float sdz = (float)s0, sdzx = (float)s1;
            if (o0) o0[c] = accumulate ? po0 + sdzx : sdzx;
            if (o1) o1[c] = accumulate ? po1 + sdz : sdz;
            o2[c] = (float)(s0 * invM);
            o2[C + c] = (float)(s1 * invM);
        }
    }
    if (MODE == 1 && bp.out) {
        float dzmax = pdz;                                       // (every thread: the shuffles need whole waves)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dzmax = fmaxf(dzmax, __shfl_xor(dzmax, o, 64));
        float b = 0.f;
        if (tid < 16 && c < C)
            b = fabsf(psc) * (dzmax + fabsf((float)(s0 * invM)) + fabsf((float)(s1 * invM)) * bp.sqrtM);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) b = fmaxf(b, __shfl_xor(b, o, 64));
        if (tid == 0 && b > 0.f) atomicMax(bp.out + (wg & 63), __float_as_uint(b));
    }
}

extern "C" int dsnt_bn_finalize(const float* partial, int ntiles, int64_t M, int C,
                                const float* gamma, const float* beta, float* running_mean,
                                float* running_var, float momentum, float eps, int training,
                                float* mean, float* invstd, float* scale, float* shift,
                                void* stream) {
    DSNT_REQUIRE(mean && invstd && scale && shift && C > 0 && M > 0, DSNT_ERR_ARG,
                 "dsnt_bn_finalize: bad argument");
    DSNT_REQUIRE(training ? (partial != nullptr && ntiles > 0) : (running_mean && running_var),
                 DSNT_ERR_ARG, "dsnt_bn_finalize: missing statistics source");
    DSNT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), DSNT_ERR_ARG,
                 "dsnt_bn_finalize: running_mean/var must be given together");
    const double unbias = M > 1 ? (double)M / (double)(M - 1) : 1.0;
    const BnFinP q{partial, ntiles, 1.0 / (double)M, unbias, C, gamma, beta, running_mean, running_var, momentum, eps, training,
                   mean, invstd, scale, shift, 0, BnBoundP{nullptr, nullptr, 0.f, nullptr}};
    DSNT_LAUNCH(bn_finalize_kernel<0>, dim3((C + 15) / 16), dim3(FIN_T), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_bn_finalize");
}

// Eval-mode BatchNorm vectors of MANY layers in one launch (table rows of int64: {gamma*, beta*, running_mean*,
// running_var*, mean*, invstd*, scale*, shift*, C, bits of float eps}): what dsnt_bn_finalize(training = 0) computes per
// layer — 96 launches per hg2 forward otherwise, the larger part of a batch-1 inference (inference.py:33-48).
__global__ __launch_bounds__(256) void bn_eval_prep_kernel(const long long* __restrict__ table) {
    const long long* t = table + (size_t)blockIdx.x * 10;
    const float* gamma = reinterpret_cast<const float*>(t[0]);
    const float* beta = reinterpret_cast<const float*>(t[1]);
    const float* rm = reinterpret_cast<const float*>(t[2]);
    const float* rv = reinterpret_cast<const float*>(t[3]);
    float* mean = reinterpret_cast<float*>(t[4]);
    float* invstd = reinterpret_cast<float*>(t[5]);
    float* scale = reinterpret_cast<float*>(t[6]);
    float* shift = reinterpret_cast<float*>(t[7]);
    const int C = (int)t[8];
    const float eps = __uint_as_float((unsigned)t[9]);
    for (int c = threadIdx.x; c < C; c += 256) {
        const double var = rv[c];
        const float is = (float)(1.0 / sqrt(var + (double)eps));
        const float mu = rm[c];
        const float sc = gamma ? gamma[c] * is : is;
        mean[c] = mu; invstd[c] = is; scale[c] = sc;
        shift[c] = (beta ? beta[c] : 0.f) - mu * sc;
    }
}

extern "C" int dsnt_bn_eval_prep(const int64_t* table, int rows, void* stream) {
    DSNT_REQUIRE(table && rows > 0, DSNT_ERR_ARG, "dsnt_bn_eval_prep: bad argument");
    DSNT_LAUNCH(bn_eval_prep_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, (const long long*)table);
    DSNT_CHECK_LAUNCH("dsnt_bn_eval_prep");
}

extern "C" int dsnt_bn_bwd_finalize(const float* partial, int ntiles, int64_t M, int C,
                                    float* dgamma, float* dbeta, int accumulate, float* coef,
                                    void* stream) {
    DSNT_REQUIRE(partial && coef && ntiles > 0 && C > 0 && M > 0, DSNT_ERR_ARG,
                 "dsnt_bn_bwd_finalize: bad argument");
    // DSNT_BN_FROZEN: the forward ran on fixed (running) statistics — dx = scale dz, both coefficients zero; dgamma / dbeta as always
    const double invM = (accumulate & DSNT_BN_FROZEN) ? 0.0 : 1.0 / (double)M;
    const BnFinP q{partial, ntiles, invM, 1.0, C, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 1, dgamma, dbeta, coef, nullptr,
                   accumulate & 1, BnBoundP{nullptr, nullptr, 0.f, nullptr}};
    DSNT_LAUNCH(bn_finalize_kernel<1>, dim3((C + 15) / 16), dim3(FIN_T), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_bn_bwd_finalize");
}

// dsnt_bn_bwd_finalize that also leaves the bound of the BatchNorm's dx for a consumer that never sees dx in memory
// (dsnt_conv1x1_bwd_f16x3 with a dsnt_bn_bwd_apply): scale = the BatchNorm's forward scale vector (gamma * invstd), dz_amax = the
// 64-slot max |dz| its data-gradient producer left (dsnt_out_bounds.amax), bound_out = 64 slots, zeroed by the caller once per step.
extern "C" int dsnt_bn_bwd_finalize_bound(const float* partial, int ntiles, int64_t M, int C, float* dgamma, float* dbeta,
                                          int accumulate, float* coef, const float* scale, const float* dz_amax,
                                          float* bound_out, void* stream) {
    DSNT_REQUIRE(partial && coef && scale && dz_amax && bound_out && ntiles > 0 && C > 0 && M > 0, DSNT_ERR_ARG,
                 "dsnt_bn_bwd_finalize_bound: bad argument");
    // a frozen BatchNorm has no folded apply (dx = scale dz needs no bound of the coefficients): the flag is refused, not read as bit 0
    DSNT_REQUIRE(!(accumulate & DSNT_BN_FROZEN), DSNT_ERR_ARG, "dsnt_bn_bwd_finalize_bound: DSNT_BN_FROZEN has no bound form");
    const BnFinP q{partial, ntiles, 1.0 / (double)M, 1.0, C, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 1, dgamma, dbeta, coef, nullptr,
                   accumulate & 1, BnBoundP{scale, dz_amax, sqrtf((float)M), reinterpret_cast<unsigned*>(bound_out)}};
    DSNT_LAUNCH(bn_finalize_kernel<1>, dim3((C + 15) / 16), dim3(FIN_T), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_bn_bwd_finalize_bound");
}

// ---------------------------------------------------------------- apply, forward
__global__ void bn_act_fwd_kernel(const float4* __restrict__ x, const float4* __restrict__ scale,
                                  const float4* __restrict__ shift, int relu, float4* __restrict__ y,
                                  long n4, int C4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        const float4 v = x[i], sc = scale[cg], sh = shift[cg];
        float4 o = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z),
                               fmaf(v.w, sc.w, sh.w));
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        y[i] = o;
    }
}

extern "C" int dsnt_bn_act_fwd(const float* x, const float* scale, const float* shift, int relu,
                               float* y, int64_t M, int C, void* stream) {
    DSNT_REQUIRE(x && scale && shift && y && M > 0 && C > 0, DSNT_ERR_ARG, "dsnt_bn_act_fwd: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(y) && dsnt_aligned16(scale) &&
                 dsnt_aligned16(shift), DSNT_ERR_ALIGN, "dsnt_bn_act_fwd: alignment");
    const long n4 = (long)M * C / 4;
    DSNT_LAUNCH(bn_act_fwd_kernel, dim3(flat_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)x, (const float4*)scale, (const float4*)shift, relu, (float4*)y,
                       n4, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_bn_act_fwd");
}

// y = relu?(scale * x + shift + res): the tail of a torchvision BasicBlock / Bottleneck (bn -> += identity -> relu)
__global__ void bn_add_act_fwd_kernel(const float4* __restrict__ x, const float4* __restrict__ scale,
                                      const float4* __restrict__ shift, const float4* __restrict__ res, int relu,
                                      float4* __restrict__ y, long n4, int C4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        const float4 v = x[i], sc = scale[cg], sh = shift[cg], r = res[i];
        float4 o = make_float4(fmaf(v.x, sc.x, sh.x) + r.x, fmaf(v.y, sc.y, sh.y) + r.y, fmaf(v.z, sc.z, sh.z) + r.z,
                               fmaf(v.w, sc.w, sh.w) + r.w);
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        y[i] = o;
    }
}

extern "C" int dsnt_bn_add_act_fwd(const float* x, const float* scale, const float* shift, const float* res,
                                   int relu, float* y, int64_t M, int C, void* stream) {
    DSNT_REQUIRE(x && scale && shift && res && y && M > 0 && C > 0, DSNT_ERR_ARG, "dsnt_bn_add_act_fwd: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(y) && dsnt_aligned16(res) && dsnt_aligned16(scale) &&
                 dsnt_aligned16(shift), DSNT_ERR_ALIGN, "dsnt_bn_add_act_fwd: alignment");
    const long n4 = (long)M * C / 4;
    DSNT_LAUNCH(bn_add_act_fwd_kernel, dim3(flat_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)x, (const float4*)scale, (const float4*)shift, (const float4*)res, relu,
                       (float4*)y, n4, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_bn_add_act_fwd");
}

// dz = dy where y > 0, else 0 (backward of the block-output ReLU; ATen's threshold_backward keeps dy for y > 0)
__global__ void relu_bwd_kernel(const float4* __restrict__ dy, const float4* __restrict__ y, float4* __restrict__ dz,
                                long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 g = dy[i], v = y[i];
        dz[i] = make_float4(v.x > 0.f ? g.x : 0.f, v.y > 0.f ? g.y : 0.f, v.z > 0.f ? g.z : 0.f, v.w > 0.f ? g.w : 0.f);
    }
}

extern "C" int dsnt_relu_bwd(const float* dy, const float* y, float* dz, int64_t n, void* stream) {
    DSNT_REQUIRE(dy && y && dz && n > 0 && n % 4 == 0, DSNT_ERR_ARG, "dsnt_relu_bwd: bad argument");
    DSNT_REQUIRE(dsnt_aligned16(dy) && dsnt_aligned16(y) && dsnt_aligned16(dz), DSNT_ERR_ALIGN, "dsnt_relu_bwd: alignment");
    DSNT_LAUNCH(relu_bwd_kernel, dim3(flat_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)dy, (const float4*)y, (float4*)dz, (long)(n / 4));
    DSNT_CHECK_LAUNCH("dsnt_relu_bwd");
}

// ---------------------------------------------------------------- apply, backward
// FIXED: the grid stride is a multiple of C/4, so a thread stays on ONE channel group — its six per-channel vectors are
// loaded once instead of with every element (they were two thirds of the kernel's load instructions), and two elements are
// in flight per iteration.  Same arithmetic, element for element.
struct BnApplyVec { float4 sc, sh, mu, is, c0, c1; };
__device__ __forceinline__ float4 bn_apply_one(const float4 g, const float4 xv, const BnApplyVec& v, int relu) {
    float4 dz = g;
    if (relu) {
        if (fmaf(xv.x, v.sc.x, v.sh.x) <= 0.f) dz.x = 0.f;
        if (fmaf(xv.y, v.sc.y, v.sh.y) <= 0.f) dz.y = 0.f;
        if (fmaf(xv.z, v.sc.z, v.sh.z) <= 0.f) dz.z = 0.f;
        if (fmaf(xv.w, v.sc.w, v.sh.w) <= 0.f) dz.w = 0.f;
    }
    float4 o;
    o.x = v.sc.x * (dz.x - v.c0.x - (xv.x - v.mu.x) * v.is.x * v.c1.x);
    o.y = v.sc.y * (dz.y - v.c0.y - (xv.y - v.mu.y) * v.is.y * v.c1.y);
    o.z = v.sc.z * (dz.z - v.c0.z - (xv.z - v.mu.z) * v.is.z * v.c1.z);
    o.w = v.sc.w * (dz.w - v.c0.w - (xv.w - v.mu.w) * v.is.w * v.c1.w);
    return o;
}
struct BnApplyP {
    const float4* da; const float4* x; const float4* scale; const float4* shift; const float4* mean; const float4* invstd;
    const float4* coef; int relu; float4* dx; const float4* base; long n4; int C4; unsigned* amax; BnBwdProP pro;
};
template <bool FIXED>
__global__ void bn_act_bwd_apply_kernel(BnApplyP q) {
    __shared__ double pro_sh[512];
    const float4* __restrict__ da = q.da; const float4* __restrict__ x = q.x; const float4* __restrict__ scale = q.scale;
    const float4* __restrict__ shift = q.shift; const float4* __restrict__ mean = q.mean; const float4* __restrict__ invstd = q.invstd;
    const float4* coef = q.coef; const int relu = q.relu; float4* dx = q.dx; const float4* base = q.base;
    const long n4 = q.n4; const int C4 = q.C4; unsigned* __restrict__ amax = q.amax; const BnBwdProP pro = q.pro;
    // base: what the result is added to — null (dx = value), dx itself (accumulate in place) or ANOTHER tensor (dx = base + value:
    // the gradient it continues stays intact for a reader that comes later, dsnt_bn_act_bwd_apply_base)
    const bool accumulate = base != nullptr;
    const int wg = blockIdx.x, nwg = gridDim.x;
    if (pro.partial) {                   // dsnt_bn_act_bwd_apply_pro: coef / dgamma / dbeta from the tile sums, here
        bn_pro_backward<256>(pro, pro_sh, wg == 0);
        __syncthreads();                 // this workgroup's stores to coef are visible to its loads below
    }
    float am = 0.f;
    const long stride = (long)nwg * 256;
    // (256 threads per workgroup: the select always takes its first arm.  Without it <true> needs 4 more VGPRs, <false> 3 more instructions)
    long i = threadIdx.x < 256 ? (long)wg * 256 + threadIdx.x : n4;
    auto vec = [&](int cg) {
        BnApplyVec v;
        v.sc = scale[cg]; v.sh = shift[cg]; v.mu = mean[cg]; v.is = invstd[cg]; v.c0 = coef[cg]; v.c1 = coef[C4 + cg];
        return v;
    };
    auto amx = [&](const float4 o) { am = fmaxf(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))), am); };
    if (FIXED) {
        const BnApplyVec v = vec((int)((i < n4 ? i : 0) % C4));
        for (; i + stride < n4; i += 2 * stride) {
            const float4 g0 = da[i], x0 = x[i], g1 = da[i + stride], x1 = x[i + stride];
            float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0;
            if (accumulate) { p0 = base[i]; p1 = base[i + stride]; }
            float4 o0 = bn_apply_one(g0, x0, v, relu), o1 = bn_apply_one(g1, x1, v, relu);
            if (accumulate) {
                o0.x += p0.x; o0.y += p0.y; o0.z += p0.z; o0.w += p0.w;
                o1.x += p1.x; o1.y += p1.y; o1.z += p1.z; o1.w += p1.w;
            }
            dx[i] = o0; dx[i + stride] = o1;
            amx(o0); amx(o1);
        }
        if (i < n4) {
            float4 o = bn_apply_one(da[i], x[i], v, relu);
            if (accumulate) { const float4 p = base[i]; o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
            dx[i] = o;
            amx(o);
        }
    } else {
        for (; i < n4; i += stride) {
            float4 o = bn_apply_one(da[i], x[i], vec((int)(i % C4)), relu);
            if (accumulate) { const float4 p = base[i]; o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
            dx[i] = o;
            amx(o);
        }
    }
    if (amax) amax_commit(am, amax);             // max |dx| for the fp16x3 consumers
}

static int bn_act_bwd_apply_impl(const float* da, const float* x, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, const float* coef, int relu, float* dx,
                                 int accumulate, int64_t M, int C, float* amax, void* stream, const BnBwdProP* pro, const float* base) {
    DSNT_REQUIRE(da && x && scale && shift && mean && invstd && coef && dx && M > 0 && C > 0,
                 DSNT_ERR_ARG, "dsnt_bn_act_bwd_apply: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(da) && dsnt_aligned16(x) && dsnt_aligned16(dx) &&
                 dsnt_aligned16(coef) && dsnt_aligned16(base), DSNT_ERR_ALIGN, "dsnt_bn_act_bwd_apply: alignment");
    if (!base && accumulate) base = dx;
    const long n4 = (long)M * C / 4;
    int grid = flat_grid(n4, 256);
    BnBwdProP q;
    memset(&q, 0, sizeof(q));
    if (pro) {
        q = *pro;
        // every workgroup re-reads the tile sums in its prologue: few, fat workgroups (these launches are latency-bound)
        if (grid > 128) grid = 128;
    }
    const BnApplyP ap{(const float4*)da, (const float4*)x, (const float4*)scale, (const float4*)shift, (const float4*)mean,
                      (const float4*)invstd, (const float4*)coef, relu, (float4*)dx, (const float4*)base, n4, C / 4, (unsigned*)amax, q};
    if (((long)grid * 256) % (C / 4) == 0)
        DSNT_LAUNCH(bn_act_bwd_apply_kernel<true>, dim3(grid), dim3(256), 0, stream, ap);
    else
        DSNT_LAUNCH(bn_act_bwd_apply_kernel<false>, dim3(grid), dim3(256), 0, stream, ap);
    DSNT_CHECK_LAUNCH("dsnt_bn_act_bwd_apply");
}

extern "C" int dsnt_bn_act_bwd_apply_amax(const float* da, const float* x, const float* scale,
                                          const float* shift, const float* mean, const float* invstd,
                                          const float* coef, int relu, float* dx, int accumulate,
                                          int64_t M, int C, float* amax, void* stream) {
    return bn_act_bwd_apply_impl(da, x, scale, shift, mean, invstd, coef, relu, dx, accumulate, M, C, amax, stream, nullptr, nullptr);
}

extern "C" int dsnt_bn_act_bwd_apply(const float* da, const float* x, const float* scale,
                                     const float* shift, const float* mean, const float* invstd,
                                     const float* coef, int relu, float* dx, int accumulate,
                                     int64_t M, int C, void* stream) {
    return bn_act_bwd_apply_impl(da, x, scale, shift, mean, invstd, coef, relu, dx, accumulate, M, C, nullptr, stream, nullptr, nullptr);
}

// The tile sums a prologue reads (bn_pro.h: bn_pro_backward), checked and packed for the two _pro entries; `who` names the entry.
static int bn_bwd_pro_fill(BnBwdProP& q, const char* who, const float* partial, int ntiles, float* dgamma, float* dbeta,
                           int accumulate_params, float* coef, int64_t M, int C) {
    DSNT_REQUIRE(partial && ntiles > 0 && coef && C <= 256 && (long)ntiles * C <= 16384, DSNT_ERR_ARG,
                 "%s: needs partial sums of at most 256 channels / 128 KB and a coef buffer", who);
    q.partial = partial; q.tiles = ntiles; q.C = C; q.invM = 1.0 / (double)M;
    q.dgamma = dgamma; q.dbeta = dbeta; q.accumulate = accumulate_params; q.coef = coef;
    return DSNT_OK;
}

// The same with dsnt_bn_bwd_finalize folded into its prologue (tile sums of <= 64 KB: the 8x8 / 4x4 hourglass levels,
// where a finalise launch between two 10-us kernels costs the chain ~8 us): every workgroup sums partial[tiles][2][C]
// itself (fp64, fixed order) into coef, workgroup 0 also writes dgamma / dbeta (+= with accumulate_params).
extern "C" int dsnt_bn_act_bwd_apply_pro(const float* da, const float* x, const float* scale, const float* shift,
                                         const float* mean, const float* invstd, const float* partial, int ntiles,
                                         float* dgamma, float* dbeta, int accumulate_params, float* coef, int relu,
                                         float* dx, int accumulate, int64_t M, int C, float* amax, void* stream) {
    BnBwdProP q;
    if (int e = bn_bwd_pro_fill(q, "dsnt_bn_act_bwd_apply_pro", partial, ntiles, dgamma, dbeta, accumulate_params, coef, M, C)) return e;
    return bn_act_bwd_apply_impl(da, x, scale, shift, mean, invstd, coef, relu, dx, accumulate, M, C, amax, stream, &q, nullptr);
}
// dx = base + value with `base` a tensor of its own (read, never written): the gradient that dx continues stays intact — for a
// weight gradient that reads it at the end of its parameter bucket (the grouped launch), after dx has long been written.
// amax may be NULL.  The _pro form: dsnt_bn_act_bwd_apply_pro likewise.
extern "C" int dsnt_bn_act_bwd_apply_base(const float* da, const float* x, const float* scale, const float* shift,
                                          const float* mean, const float* invstd, const float* coef, int relu,
                                          const float* base, float* dx, int64_t M, int C, float* amax, void* stream) {
    DSNT_REQUIRE(base && base != dx, DSNT_ERR_ARG, "dsnt_bn_act_bwd_apply_base: `base` must be a second tensor");
    return bn_act_bwd_apply_impl(da, x, scale, shift, mean, invstd, coef, relu, dx, 1, M, C, amax, stream, nullptr, base);
}
extern "C" int dsnt_bn_act_bwd_apply_pro_base(const float* da, const float* x, const float* scale, const float* shift,
                                              const float* mean, const float* invstd, const float* partial, int ntiles,
                                              float* dgamma, float* dbeta, int accumulate_params, float* coef, int relu,
                                              const float* base, float* dx, int64_t M, int C, float* amax, void* stream) {
    DSNT_REQUIRE(base && base != dx, DSNT_ERR_ARG, "dsnt_bn_act_bwd_apply_pro_base: `base` must be a second tensor");
    BnBwdProP q;
    if (int e = bn_bwd_pro_fill(q, "dsnt_bn_act_bwd_apply_pro_base", partial, ntiles, dgamma, dbeta, accumulate_params, coef, M, C)) return e;
    return bn_act_bwd_apply_impl(da, x, scale, shift, mean, invstd, coef, relu, dx, 1, M, C, amax, stream, &q, base);
}
