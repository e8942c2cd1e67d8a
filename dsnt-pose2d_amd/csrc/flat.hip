// Flat grid-stride kernels with no per-channel state: zero fill, axpy (the gradient accumulations of autograd), the
// NCHW <-> NHWC layout changes at the model's boundary and the space-to-depth operands of the 7x7 stem (hourglass.py:106).
#include "common.h"

__global__ void fill_zero_kernel(float* p, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = 0.f;
}

extern "C" int dsnt_fill_zero(float* p, int64_t n, void* stream) {
    DSNT_REQUIRE(p && n > 0, DSNT_ERR_ARG, "dsnt_fill_zero: bad argument");
    DSNT_LAUNCH(fill_zero_kernel, dim3(flat_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, (long)n);
    DSNT_CHECK_LAUNCH("dsnt_fill_zero");
}

__global__ void axpy_kernel(const float* __restrict__ x, float* y, float a, int accumulate, long n, unsigned* amax) {
    const long n4 = n >> 2;
    float am = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        float4 o = make_float4(a * v.x, a * v.y, a * v.z, a * v.w);
        if (accumulate) {
            const float4 c = reinterpret_cast<float4*>(y)[i];
            o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w;
        }
        reinterpret_cast<float4*>(y)[i] = o;
        am = fmaxf(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))), am);
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        const float o = accumulate ? y[i] + a * x[i] : a * x[i];
        y[i] = o;
        am = fmaxf(am, fabsf(o));
    }
    if (amax) amax_commit(am, amax);
}

static int axpy_impl(const float* x, float* y, float a, int accumulate, int64_t n, float* amax, void* stream) {
    DSNT_REQUIRE(x && y && n > 0, DSNT_ERR_ARG, "dsnt_axpy: bad argument");
    DSNT_REQUIRE(dsnt_aligned16(x) && dsnt_aligned16(y), DSNT_ERR_ALIGN, "dsnt_axpy: alignment");
    DSNT_LAUNCH(axpy_kernel, dim3(flat_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, x, y,
                       a, accumulate, (long)n, (unsigned*)amax);
    DSNT_CHECK_LAUNCH("dsnt_axpy");
}
extern "C" int dsnt_axpy(const float* x, float* y, float a, int accumulate, int64_t n, void* stream) {
    return axpy_impl(x, y, a, accumulate, n, nullptr, stream);
}
extern "C" int dsnt_axpy_amax(const float* x, float* y, float a, int accumulate, int64_t n, float* amax, void* stream) {
    return axpy_impl(x, y, a, accumulate, n, amax, stream);
}

// ---------------------------------------------------------------- layout changes
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C,
                                    int HW, int Cpad) {
    const long total = (long)N * HW;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const long n = i / HW;
        for (int c = 0; c < Cpad; ++c)
            dst[i * Cpad + c] = c < C ? src[(n * C + c) * HW + p] : 0.f;
    }
}
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C,
                                    int HW, int Cpad) {
    const long total = (long)N * HW;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const long n = i / HW;
        for (int c = 0; c < C; ++c) dst[(n * C + c) * HW + p] = src[i * Cpad + c];
    }
}

extern "C" int dsnt_nchw_to_nhwc(const float* src, float* dst, int N, int C, int HW, int Cpad, void* stream) {
    DSNT_REQUIRE(src && dst && N > 0 && C > 0 && HW > 0 && Cpad >= C, DSNT_ERR_ARG, "dsnt_nchw_to_nhwc: bad argument");
    DSNT_LAUNCH(nchw_to_nhwc_kernel, dim3(flat_grid((long)N * HW, 256)), dim3(256), 0,
                       (hipStream_t)stream, src, dst, N, C, HW, Cpad);
    DSNT_CHECK_LAUNCH("dsnt_nchw_to_nhwc");
}
extern "C" int dsnt_nhwc_to_nchw(const float* src, float* dst, int N, int C, int HW, int Cpad, void* stream) {
    DSNT_REQUIRE(src && dst && N > 0 && C > 0 && HW > 0 && Cpad >= C, DSNT_ERR_ARG, "dsnt_nhwc_to_nchw: bad argument");
    DSNT_LAUNCH(nhwc_to_nchw_kernel, dim3(flat_grid((long)N * HW, 256)), dim3(256), 0,
                       (hipStream_t)stream, src, dst, N, C, HW, Cpad);
    DSNT_CHECK_LAUNCH("dsnt_nhwc_to_nchw");
}

// ---------------------------------------------------------------- 7x7 / stride 2 stem as a 4x4 / stride 1 convolution
// The stem (hourglass.py:106 / torchvision's conv1: 7x7, stride 2, pad 3 on a 3-channel image) has K = 7*7*4 = 196 with four
// channels per tap — nothing the 16-channel K-steps of the split-precision kernels can use, so it ran on the fp32 MFMA at a
// third of that pipe's peak.  Space-to-depth turns it into an ordinary convolution: 2x2 pixel blocks become 16 channels
// ((dy*2+dx)*4 + c), the 7x7 filter — extended by a zero row and column at the TOP / LEFT to 8x8 — becomes 4x4 block taps at
// block offsets -2..+1, and with one zero block row / column in front of the image that is a 4x4, stride 1, pad 1 convolution
// on [N][H/2+1][W/2+1][16]: K = 256 (23 % zeros), every large-tile fp16x3 / bf16x6 kernel applies.
//   dst[n][1+i][1+j][(dy*2+dx)*4 + c] = src[n][c][2i+dy][2j+dx]   (c < C <= 4; channel C..3, block row 0, block column 0: zero)
__global__ void s2d_input_kernel(const float* __restrict__ src, float4* __restrict__ dst, int N, int C, int H, int W,
                                 unsigned* __restrict__ amax) {
    const int Hb = H / 2 + 1, Wb = W / 2 + 1;
    const long total = (long)N * Hb * Wb * 4;             // one float4 (= one pixel of a block) per item
    float am = 0.f;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int q = (int)(t & 3);                       // dy*2 + dx
        long b = t >> 2;
        const int j = (int)(b % Wb); b /= Wb;
        const int i = (int)(b % Hb);
        const long n = b / Hb;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i > 0 && j > 0) {
            const int y = 2 * (i - 1) + (q >> 1), x = 2 * (j - 1) + (q & 1);
            const float* s0 = src + ((n * C) * H + y) * (long)W + x;
            v.x = s0[0];
            if (C > 1) v.y = s0[(long)H * W];
            if (C > 2) v.z = s0[2l * H * W];
            if (C > 3) v.w = s0[3l * H * W];
        }
        dst[t] = v;
        am = fmaxf(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))), am);
    }
    if (amax) amax_commit(am, amax);
}

extern "C" int dsnt_s2d_input(const float* src_nchw, float* dst, int N, int C, int H, int W, const dsnt_out_bounds* tail,
                              void* stream) {
    DSNT_REQUIRE(src_nchw && dst && N > 0 && C > 0 && C <= 4 && H > 0 && W > 0, DSNT_ERR_ARG, "dsnt_s2d_input: bad argument");
    DSNT_REQUIRE(H % 2 == 0 && W % 2 == 0, DSNT_ERR_SHAPE, "dsnt_s2d_input: H and W must be even (got %dx%d)", H, W);
    DSNT_REQUIRE(dsnt_aligned16(dst), DSNT_ERR_ALIGN, "dsnt_s2d_input: dst must be 16-byte aligned");
    const long total = (long)N * (H / 2 + 1) * (W / 2 + 1) * 4;
    DSNT_LAUNCH(s2d_input_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, src_nchw, (float4*)dst, N, C,
                H, W, (unsigned*)(tail ? tail->amax : nullptr));
    DSNT_CHECK_LAUNCH("dsnt_s2d_input");
}

// w2[co][R][S][(dy*2+dx)*4 + c] = w[co][2R+dy-1][2S+dx-1][c] (OHWI, 4 stored channels; 0 outside the 7x7);  back != 0: the
// inverse gather for the weight gradient, dw[co][r][s][c] = dw2[co][(r+1)/2][(s+1)/2][(((r+1)&1)*2 + ((s+1)&1))*4 + c].
__global__ void s2d_weights_kernel(const float* __restrict__ w, float* __restrict__ w2, int Cout, int back) {
    const int total = back ? Cout * 49 * 4 : Cout * 256;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        if (back) {
            const int c = t & 3, rs = (t >> 2) % 49, co = (t >> 2) / 49;
            const int r = rs / 7 + 1, s_ = rs % 7 + 1;
            w2[t] = w[((co * 4 + (r >> 1)) * 4 + (s_ >> 1)) * 16 + ((r & 1) * 2 + (s_ & 1)) * 4 + c];
        } else {
            const int k = t & 15, S = (t >> 4) & 3, R = (t >> 6) & 3, co = t >> 8;
            const int c = k & 3, dx = (k >> 2) & 1, dy = k >> 3;
            const int r = 2 * R + dy - 1, s_ = 2 * S + dx - 1;
            w2[t] = (r >= 0 && s_ >= 0) ? w[((co * 7 + r) * 7 + s_) * 4 + c] : 0.f;
        }
    }
}

extern "C" int dsnt_s2d_weights(const float* w, float* w2, int Cout, int back, void* stream) {
    DSNT_REQUIRE(w && w2 && Cout > 0, DSNT_ERR_ARG, "dsnt_s2d_weights: bad argument");
    const int total = back ? Cout * 196 : Cout * 256;
    DSNT_LAUNCH(s2d_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, w2, Cout, back);
    DSNT_CHECK_LAUNCH("dsnt_s2d_weights");
}
