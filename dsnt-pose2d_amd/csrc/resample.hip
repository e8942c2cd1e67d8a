// Resolution changes on NHWC: the hourglass's 2x2 max-pool and nearest-upsample + add (hourglass.py:58, 80, 111), forward
// (plain, and with the BatchNorm statistics of the output in the same pass) and backward; torchvision's 3x3 / stride 2
// max-pool; the zero-insert of a strided data gradient.  All 16-byte vectorised (C % 4 == 0), grid-stride or one
// workgroup per 128-row tile.
#include "common.h"
#include "bn_pro.h"
#include "ew_bodies.h"

// ---------------------------------------------------------------- pooling / upsampling
__global__ void maxpool2_fwd_kernel(const float4* __restrict__ x, float4* __restrict__ y,
                                    uchar4* __restrict__ idx, int N, int H, int W, int C4) {
    const int Ho = H >> 1, Wo = W >> 1;
    const long total = (long)N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const float4* base = x + (((long)n * H + 2 * oh) * W + 2 * ow) * C4 + cg;
        const float4 v0 = base[0], v1 = base[C4], v2 = base[(long)W * C4], v3 = base[(long)W * C4 + C4];
        float4 m = v0;
        uchar4 k = make_uchar4(0, 0, 0, 0);
#define POOL_STEP(V, P)                                  \
        if (V.x > m.x || V.x != V.x) { m.x = V.x; k.x = P; } \
        if (V.y > m.y || V.y != V.y) { m.y = V.y; k.y = P; } \
        if (V.z > m.z || V.z != V.z) { m.z = V.z; k.z = P; } \
        if (V.w > m.w || V.w != V.w) { m.w = V.w; k.w = P; }
        POOL_STEP(v1, 1) POOL_STEP(v2, 2) POOL_STEP(v3, 3)
#undef POOL_STEP
        y[i] = m;
        idx[i] = k;
    }
}

extern "C" int dsnt_maxpool2_fwd(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C,
                                 void* stream) {
    DSNT_REQUIRE(x && y && idx && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG, "dsnt_maxpool2_fwd: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_maxpool2_fwd: H and W must be even (got %dx%d)", H, W);
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(y) && (((uintptr_t)idx) & 3) == 0,
                 DSNT_ERR_ALIGN, "dsnt_maxpool2_fwd: alignment");
    const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
    DSNT_LAUNCH(maxpool2_fwd_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)x, (float4*)y, (uchar4*)idx, N, H, W, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_maxpool2_fwd");
}

// 2x2 max-pool / nearest-upsample + add with the BatchNorm statistics of their OUTPUT in the same pass: one
// workgroup per 128 output rows (pixels), same thread mapping, accumulation order and partial format as
// tile_reduce_kernel<0>, so the sums are bit-identical to a separate dsnt_bn_stats over the stored tensor (which
// cost one more read of it: 18 launches per hg2 step).  OP 0: y = maxpool2(a) (+ arg-max byte), a is [N][2Ho][2Wo][C];
// OP 1: y = a + upsample2(b), b is [N][Ho/2][Wo/2][C].  OP 2: y = relu?(a * bn_scale + bn_shift) (the stem's materialised
// BatchNorm + ReLU, hourglass.py:157-159).  Ho, Wo: OUTPUT size.
extern "C" int dsnt_maxpool2_fwd_stats(const float* x, float* y, uint8_t* idx, float* partial, int N, int H, int W,
                                       int C, const dsnt_out_bounds* g_tail, void* stream) {
    OutBoundsP tail;
    if (int e = out_bounds_fill(tail, g_tail, "dsnt_maxpool2_fwd_stats")) return e;
    DSNT_REQUIRE(x && y && idx && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG,
                 "dsnt_maxpool2_fwd_stats: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_maxpool2_fwd_stats: H and W must be even (got %dx%d)", H, W);
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(y) && dsnt_aligned16(partial) &&
                 (((uintptr_t)idx) & 3) == 0, DSNT_ERR_ALIGN, "dsnt_maxpool2_fwd_stats: alignment");
    const long M = (long)N * (H / 2) * (W / 2);
    const long tiles = (M + TILE_ROWS - 1) / TILE_ROWS;
    const TileOpP q{x, nullptr, y, idx, partial, N, H / 2, W / 2, C, tile_cgs(tiles, C / 4), tail, nullptr, nullptr, 0};
    DSNT_LAUNCH(tile_op_stats_kernel<0>, dim3((unsigned)tiles, tile_grid_y(tiles, C / 4)), dim3(256), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_maxpool2_fwd_stats");
}

// (`extra`, optional: a second gradient of x — same layout as dx — added in the same pass: dx (+)= extra + the routed dy)
struct PoolBwdP { const float4* dy; const uchar4* idx; float4* dx; int accumulate; const float4* extra; int N, H, W, C4; unsigned* amax; };
__global__ void maxpool2_bwd_kernel(PoolBwdP q) {
    const float4* __restrict__ dy = q.dy; const uchar4* __restrict__ idx = q.idx; float4* dx = q.dx; const int accumulate = q.accumulate;
    const float4* __restrict__ extra = q.extra; const int H = q.H, W = q.W, C4 = q.C4, N = q.N; unsigned* amax = q.amax;
    const int Ho = H >> 1, Wo = W >> 1;
    const long total = (long)N * Ho * Wo * C4;
    const int wg = blockIdx.x, nwg = gridDim.x;
    float am = 0.f;
    for (long i = (long)wg * 256 + threadIdx.x; i < total; i += (long)nwg * 256) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const float4 g = dy[i];
        const uchar4 k = idx[i];
        float4* base = dx + (((long)n * H + 2 * oh) * W + 2 * ow) * C4 + cg;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float4* q = base + (p >> 1) * (long)W * C4 + (p & 1) * C4;
            float4 o = make_float4(k.x == p ? g.x : 0.f, k.y == p ? g.y : 0.f, k.z == p ? g.z : 0.f,
                                   k.w == p ? g.w : 0.f);
            if (accumulate) { const float4 c = *q; o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
            if (extra) { const float4 e = extra[q - dx]; o.x += e.x; o.y += e.y; o.z += e.z; o.w += e.w; }
            *q = o;
            am = fmaxf(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))), am);
        }
    }
    if (amax) amax_commit(am, amax);
}

static int maxpool2_bwd_impl(const float* dy, const uint8_t* idx, float* dx, int accumulate, const float* extra, int N, int H, int W,
                             int C, float* amax, void* stream) {
    DSNT_REQUIRE(dy && idx && dx && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG, "dsnt_maxpool2_bwd: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_maxpool2_bwd: H and W must be even");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(dy) && dsnt_aligned16(dx), DSNT_ERR_ALIGN, "dsnt_maxpool2_bwd: alignment");
    const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
    const PoolBwdP q{(const float4*)dy, (const uchar4*)idx, (float4*)dx, accumulate, (const float4*)extra, N, H, W, C / 4, (unsigned*)amax};
    DSNT_LAUNCH(maxpool2_bwd_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_maxpool2_bwd");
}
extern "C" int dsnt_maxpool2_bwd(const float* dy, const uint8_t* idx, float* dx, int accumulate,
                                 int N, int H, int W, int C, void* stream) {
    return maxpool2_bwd_impl(dy, idx, dx, accumulate, nullptr, N, H, W, C, nullptr, stream);
}
extern "C" int dsnt_maxpool2_bwd_amax(const float* dy, const uint8_t* idx, float* dx, int accumulate,
                                      int N, int H, int W, int C, float* amax, void* stream) {
    return maxpool2_bwd_impl(dy, idx, dx, accumulate, nullptr, N, H, W, C, amax, stream);
}
extern "C" int dsnt_maxpool2_bwd_add(const float* dy, const uint8_t* idx, float* dx, int accumulate, const float* extra,
                                     int N, int H, int W, int C, float* amax, void* stream) {
    DSNT_REQUIRE(extra && extra != dx && dsnt_aligned16(extra), DSNT_ERR_ARG, "dsnt_maxpool2_bwd_add: `extra` must be a second, aligned tensor");
    return maxpool2_bwd_impl(dy, idx, dx, accumulate, extra, N, H, W, C, amax, stream);
}

__global__ void upsample2_add_fwd_kernel(const float4* __restrict__ up, const float4* __restrict__ low,
                                         float4* __restrict__ out, int N, int H, int W, int C4) {
    const long total = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int w = (int)(t % W); t /= W;
        const int h = (int)(t % H);
        const int n = (int)(t / H);
        const float4 a = up[i];
        const float4 b = low[(((long)n * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1)) * C4 + cg];
        out[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}

extern "C" int dsnt_upsample2_add_fwd(const float* up, const float* low, float* out, int N, int H,
                                      int W, int C, void* stream) {
    DSNT_REQUIRE(up && low && out && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG, "dsnt_upsample2_add_fwd: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_upsample2_add_fwd: H and W must be even");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(up) && dsnt_aligned16(low) && dsnt_aligned16(out),
                 DSNT_ERR_ALIGN, "dsnt_upsample2_add_fwd: alignment");
    const long total = (long)N * H * W * (C / 4);
    DSNT_LAUNCH(upsample2_add_fwd_kernel, dim3(flat_grid(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const float4*)up, (const float4*)low, (float4*)out, N, H, W, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_upsample2_add_fwd");
}

extern "C" int dsnt_upsample2_add_fwd_stats(const float* up, const float* low, float* out, float* partial, int N,
                                            int H, int W, int C, const dsnt_out_bounds* g_tail, void* stream) {
    OutBoundsP tail;
    if (int e = out_bounds_fill(tail, g_tail, "dsnt_upsample2_add_fwd_stats")) return e;
    DSNT_REQUIRE(up && low && out && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG,
                 "dsnt_upsample2_add_fwd_stats: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_upsample2_add_fwd_stats: H and W must be even");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(up) && dsnt_aligned16(low) && dsnt_aligned16(out) &&
                 dsnt_aligned16(partial), DSNT_ERR_ALIGN, "dsnt_upsample2_add_fwd_stats: alignment");
    const long M = (long)N * H * W;
    const long tiles = (M + TILE_ROWS - 1) / TILE_ROWS;
    const TileOpP q{up, low, out, nullptr, partial, N, H, W, C, tile_cgs(tiles, C / 4), tail, nullptr, nullptr, 0};
    DSNT_LAUNCH(tile_op_stats_kernel<1>, dim3((unsigned)tiles, tile_grid_y(tiles, C / 4)), dim3(256), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_upsample2_add_fwd_stats");
}

struct UpBwdP { const float4* dout; float4* dlow; int accumulate; int N, H, W, C4; unsigned* amax; };
__global__ void upsample2_bwd_kernel(UpBwdP q) {
    const float4* __restrict__ dout = q.dout; float4* dlow = q.dlow; const int accumulate = q.accumulate;
    const int N = q.N, H = q.H, W = q.W, C4 = q.C4; unsigned* amax = q.amax;
    const int Hl = H >> 1, Wl = W >> 1;
    const long total = (long)N * Hl * Wl * C4;
    const int wg = blockIdx.x, nwg = gridDim.x;
    float am = 0.f;
    // (256 threads per workgroup: the select always takes its first arm; without it the kernel needs one more SGPR)
    for (long i = threadIdx.x < 256 ? (long)wg * 256 + threadIdx.x : total; i < total; i += (long)nwg * 256) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int w = (int)(t % Wl); t /= Wl;
        const int h = (int)(t % Hl);
        const int n = (int)(t / Hl);
        const float4* b = dout + (((long)n * H + 2 * h) * W + 2 * w) * C4 + cg;
        const float4 v0 = b[0], v1 = b[C4], v2 = b[(long)W * C4], v3 = b[(long)W * C4 + C4];
        float4 o = make_float4((v0.x + v1.x) + (v2.x + v3.x), (v0.y + v1.y) + (v2.y + v3.y),
                               (v0.z + v1.z) + (v2.z + v3.z), (v0.w + v1.w) + (v2.w + v3.w));
        if (accumulate) { const float4 c = dlow[i]; o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
        dlow[i] = o;
        am = fmaxf(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))), am);
    }
    if (amax) amax_commit(am, amax);
}

static int upsample2_bwd_impl(const float* dout, float* dlow, int accumulate, int N, int H, int W, int C, float* amax,
                              void* stream) {
    DSNT_REQUIRE(dout && dlow && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG, "dsnt_upsample2_bwd: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_upsample2_bwd: H and W must be even");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(dout) && dsnt_aligned16(dlow), DSNT_ERR_ALIGN, "dsnt_upsample2_bwd: alignment");
    const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
    const UpBwdP q{(const float4*)dout, (float4*)dlow, accumulate, N, H, W, C / 4, (unsigned*)amax};
    DSNT_LAUNCH(upsample2_bwd_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, stream, q);
    DSNT_CHECK_LAUNCH("dsnt_upsample2_bwd");
}
extern "C" int dsnt_upsample2_bwd(const float* dout, float* dlow, int accumulate, int N, int H, int W,
                                  int C, void* stream) {
    return upsample2_bwd_impl(dout, dlow, accumulate, N, H, W, C, nullptr, stream);
}
extern "C" int dsnt_upsample2_bwd_amax(const float* dout, float* dlow, int accumulate, int N, int H, int W,
                                       int C, float* amax, void* stream) {
    return upsample2_bwd_impl(dout, dlow, accumulate, N, H, W, C, amax, stream);
}

// ---------------------------------------------------------------- ResNet pieces
// 3x3 / stride 2 / pad 1 max-pool (torchvision resnet.maxpool; reference model.py:123 keeps it in `fcn`).
// idx = winning tap 0..8 in scan order (first maximum wins, NaN propagates: ATen's max_pool2d rule).
__global__ void maxpool3s2_fwd_kernel(const float4* __restrict__ x, float4* __restrict__ y,
                                      uchar4* __restrict__ idx, int N, int H, int W, int Ho, int Wo, int C4) {
    const long total = (long)N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        uchar4 k = make_uchar4(255, 255, 255, 255);
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const int ih = 2 * oh - 1 + p / 3, iw = 2 * ow - 1 + p % 3;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            const float4 v = x[(((long)n * H + ih) * W + iw) * C4 + cg];
            // ATen: `if (val > maxval || isnan(val))`, maxindex starts at the window's first valid element
            if (k.x == 255) k.x = p;
            if (k.y == 255) k.y = p;
            if (k.z == 255) k.z = p;
            if (k.w == 255) k.w = p;
            if (v.x > m.x || v.x != v.x) { m.x = v.x; k.x = p; }
            if (v.y > m.y || v.y != v.y) { m.y = v.y; k.y = p; }
            if (v.z > m.z || v.z != v.z) { m.z = v.z; k.z = p; }
            if (v.w > m.w || v.w != v.w) { m.w = v.w; k.w = p; }
        }
        y[i] = m;
        idx[i] = k;
    }
}

extern "C" int dsnt_maxpool3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream) {
    DSNT_REQUIRE(x && y && idx && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG, "dsnt_maxpool3s2_fwd: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(x) && dsnt_aligned16(y) && (((uintptr_t)idx) & 3) == 0,
                 DSNT_ERR_ALIGN, "dsnt_maxpool3s2_fwd: alignment");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;        // floor((H + 2 - 3) / 2) + 1
    const long total = (long)N * Ho * Wo * (C / 4);
    DSNT_LAUNCH(maxpool3s2_fwd_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)x, (float4*)y, (uchar4*)idx, N, H, W, Ho, Wo, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_maxpool3s2_fwd");
}

// Gather form of the backward: every input pixel sums the gradients of the (at most 2 x 2) windows that
// picked it — no atomics, deterministic.
__global__ void maxpool3s2_bwd_kernel(const float4* __restrict__ dy, const uchar4* __restrict__ idx, float4* dx,
                                      int accumulate, int N, int H, int W, int Ho, int Wo, int C4) {
    const long total = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int iw = (int)(t % W); t /= W;
        const int ih = (int)(t % H);
        const int n = (int)(t / H);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        // windows with 2*oh - 1 <= ih <= 2*oh + 1
        for (int oh = ih / 2; oh <= (ih + 1) / 2; ++oh) {
            if (oh >= Ho) continue;
            const int r = ih - (2 * oh - 1);
            for (int ow = iw / 2; ow <= (iw + 1) / 2; ++ow) {
                if (ow >= Wo) continue;
                const int p = r * 3 + (iw - (2 * ow - 1));
                const long o = (((long)n * Ho + oh) * Wo + ow) * C4 + cg;
                const uchar4 k = idx[o];
                const float4 v = dy[o];
                if (k.x == p) g.x += v.x;
                if (k.y == p) g.y += v.y;
                if (k.z == p) g.z += v.z;
                if (k.w == p) g.w += v.w;
            }
        }
        if (accumulate) { const float4 c = dx[i]; g.x += c.x; g.y += c.y; g.z += c.z; g.w += c.w; }
        dx[i] = g;
    }
}

extern "C" int dsnt_maxpool3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int accumulate, int N, int H,
                                   int W, int C, void* stream) {
    DSNT_REQUIRE(dy && idx && dx && N > 0 && H > 0 && W > 0 && C > 0, DSNT_ERR_ARG, "dsnt_maxpool3s2_bwd: bad argument");
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(dy) && dsnt_aligned16(dx), DSNT_ERR_ALIGN, "dsnt_maxpool3s2_bwd: alignment");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long total = (long)N * H * W * (C / 4);
    DSNT_LAUNCH(maxpool3s2_bwd_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)dy, (const uchar4*)idx, (float4*)dx, accumulate, N, H, W, Ho, Wo, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_maxpool3s2_bwd");
}

// out[n][oh*s][ow*s][c] = dy[n][oh][ow][c], zeros elsewhere (out is [N][Hs][Ws][C]): the data gradient of a
// stride-s convolution is the stride-1 data gradient of this zero-stuffed tensor.
__global__ void zero_insert_kernel(const float4* __restrict__ dy, float4* __restrict__ out, int N, int Ho, int Wo,
                                   int Hs, int Ws, int s, int C4) {
    const long total = (long)N * Hs * Ws * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % C4);
        long t = i / C4;
        const int w = (int)(t % Ws); t /= Ws;
        const int h = (int)(t % Hs);
        const int n = (int)(t / Hs);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (h % s == 0 && w % s == 0 && h / s < Ho && w / s < Wo)
            v = dy[(((long)n * Ho + h / s) * Wo + w / s) * C4 + cg];
        out[i] = v;
    }
}

extern "C" int dsnt_zero_insert(const float* dy, float* out, int N, int Ho, int Wo, int C, int Hs, int Ws, int stride,
                                void* stream) {
    DSNT_REQUIRE(dy && out && N > 0 && Ho > 0 && Wo > 0 && C > 0 && stride >= 1, DSNT_ERR_ARG, "dsnt_zero_insert: bad argument");
    DSNT_REQUIRE(Hs >= (Ho - 1) * stride + 1 && Ws >= (Wo - 1) * stride + 1, DSNT_ERR_SHAPE,
                 "dsnt_zero_insert: %dx%d does not hold %dx%d at stride %d", Hs, Ws, Ho, Wo, stride);
    DSNT_REQUIRE(C % 4 == 0 && dsnt_aligned16(dy) && dsnt_aligned16(out), DSNT_ERR_ALIGN, "dsnt_zero_insert: alignment");
    const long total = (long)N * Hs * Ws * (C / 4);
    DSNT_LAUNCH(zero_insert_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)dy, (float4*)out, N, Ho, Wo, Hs, Ws, stride, C / 4);
    DSNT_CHECK_LAUNCH("dsnt_zero_insert");
}
