// Helpers shared by the convolution units: the XCD-aware block remap, the fp16x3 operand scale / 64-slot bounds, the exact
// bf16 (three-plane) and fp16 (two-plane) splits with their MFMA sequences, the kernel arguments (ConvP) and the host-side
// argument checks of the entry points.  gfx950 only.
#pragma once
#include "common.h"
#include "bn_pro.h"
#include <string.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void xcd_remap(int bid, int nwg, int& out) {
    // Blocks are dealt round-robin over the 8 XCDs; give every XCD a contiguous run of
    // tiles so neighbouring tiles (shared halo rows, shared A rows across n-tiles) meet in
    // one L2.  Bijective for any nwg (cdna guide §5, "XCD swizzle must be bijective").
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, i = bid >> 3;
    out = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}

// fp16x3 operand scale (see the fp16x3 notes at mma_split):
// 2^k with bound * 2^k in [2^13, 2^14)  (bound = m 2^E, 1 <= m < 2  ->  k = 13 - E); zero / tiny bounds are clamped
__device__ __host__ __forceinline__ float pow2_scale(float bound) {
    unsigned bits;
    memcpy(&bits, &bound, 4);
    int E = (int)((bits & 0x7fffffffu) >> 23) - 127;
    E = E < -100 ? -100 : (E > 100 ? 100 : E);
    const unsigned sb = (unsigned)(127 + 13 - E) << 23;
    float sc;
    memcpy(&sc, &sb, 4);
    return sc;
}
// A bound lives in DSNT_BOUND_SLOTS floats; its value is their maximum.  Producers that find it with atomics (the
// BN-backward apply kernel: thousands of workgroups) spread them over the slots by workgroup index: one hot address
// serialised the read-modify-writes and cost the apply kernel 30 %.
#define DSNT_BOUND_SLOTS 64
__device__ __forceinline__ float bound64(const float* __restrict__ p) {
    float b = p[threadIdx.x & 63];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = fmaxf(b, __shfl_xor(b, o, 64));
    return b;
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_f16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// 4 (already scaled) floats -> two planes of 4 fp16: 3 VALU instructions per element
__device__ __forceinline__ void split4h(const float4 v, uint2& p1, uint2& p2) {
    p1.x = pk_f16(v.x, v.y); p1.y = pk_f16(v.z, v.w);
    const f16x2v a0 = __builtin_bit_cast(f16x2v, p1.x), a1 = __builtin_bit_cast(f16x2v, p1.y);
    p2.x = pk_f16(v.x - (float)a0.x, v.y - (float)a0.y);
    p2.y = pk_f16(v.z - (float)a1.x, v.w - (float)a1.y);
}

// bf16x6: fp32-accurate convolution on the bf16 matrix cores.
// Every fp32 operand is split exactly into three bf16 planes x = x1 + x2 + x3 (8 + 8 + 8 mantissa
// bits); the product keeps the six terms of order <= 2^-16 (x1y1, x1y2, x2y1, x1y3, x2y2, x3y1),
// accumulated in the fp32 accumulator of v_mfma_f32_32x32x16_bf16.  The dropped terms are
// <= 2^-23 |xy| — below one fp32 rounding — so results match the fp32 kernel to fp32 accuracy
// (measured 2.4e-7 vs 5.4e-7 for a plain fp32 GEMM, K = 1152), at 6/16 of the fp32-MFMA cost.
// Weights are pre-split once per step (dsnt_split_bf16x3); activations are transformed
// (BN + ReLU, zero padding) and split by the loader waves while staging.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#define BK6 16
#define PITCH6 24        // bf16 per LDS row: 16 data + 8 pad = 48 B -> conflict-free ds_read_b128

__device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// 4 floats -> three planes of 4 bf16 (2 dwords each): exact 3-way split, 5.5 VALU instructions per
// element.  Deliberately NOT on packed fp32 ops: beside MFMAs a v_pk_add_f32 / v_pk_fma_f32 costs more
// issue time than the two plain instructions it replaces (MI355X_MICROARCH.md, cycle constants), and
// these kernels are bound by the SIMD's vector-issue port (their units are built with -fno-slp-vectorize).
typedef float sp_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split4(const float4 v, uint2& p1, uint2& p2, uint2& p3) {
    p1.x = pk_bf16(v.x, v.y); p1.y = pk_bf16(v.z, v.w);
    float4 r;
    r.x = v.x - __uint_as_float(p1.x << 16); r.y = v.y - __uint_as_float(p1.x & 0xffff0000u);
    r.z = v.z - __uint_as_float(p1.y << 16); r.w = v.w - __uint_as_float(p1.y & 0xffff0000u);
    p2.x = pk_bf16(r.x, r.y); p2.y = pk_bf16(r.z, r.w);
    r.x -= __uint_as_float(p2.x << 16); r.y -= __uint_as_float(p2.x & 0xffff0000u);
    r.z -= __uint_as_float(p2.y << 16); r.w -= __uint_as_float(p2.y & 0xffff0000u);
    p3.x = pk_bf16(r.x, r.y); p3.y = pk_bf16(r.z, r.w);
}

// fp16x3: the same idea on TWO fp16 planes after a power-of-two scale: x * s = h1 + h2 with h1 = fp16(x * s),
// h2 = fp16(x * s - h1) keeps 22+ significand bits, the product needs h1 g1 + h1 g2 + h2 g1 = THREE MFMAs (dropped
// term <= 2^-24 |x g|), two thirds of the LDS traffic and about half the split arithmetic of bf16x6.  Error against
// fp64 (K = 1152): 7.7e-8 of the output scale — a plain fp32 GEMM has 2.7e-7, bf16x6 5.8e-9.
// The price is fp16's exponent range: s = pow2_scale(bound) keeps |x * s| < 2^14 for any bound >= max|x| (a bound
// 64x too large costs nothing measurable; overflow would be fatal, underflow only costs absolute error
// <= 2^-38 * bound: the low plane is a multiple of 2^-24, so 2^-25 / s — attained, tests/split_ref.py).  Bounds live in device memory: BN+ReLU operands from the BN parameters (|gamma| sqrt(M) + |beta|),
// weights and BN-backward outputs from an amax their producer wrote.
// the MFMAs of one 32x32 accumulator and one 16-wide K step, smallest terms first
template <bool F16>
__device__ __forceinline__ void mma_split(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
    if (F16) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[1]), __builtin_bit_cast(f16x8, b[0]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[1]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[0]), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
    }
}

// Kernel arguments of the forward / data-gradient convolution kernels
struct ConvP {
    const float* x; const float* w; const float* bias; float* y;
    const float* in_scale; const float* in_shift;
    const float* res1; const float* res2; float* stats;
    const unsigned short* wq;      // bf16x6 path: plane 0 of the weights; planes are `wq_stride` elements apart
    long wq_stride;
    // optional batch-norm-backward epilogue (data-gradient launches): y = dz = acc * [bn(x) > 0],
    // stats = per-tile (sum dz, sum dz*xhat); the BN input x is passed through res1
    const float* bnb_scale; const float* bnb_shift; const float* bnb_mean; const float* bnb_invstd;
    int bnb_relu;
    int in_relu;
    // fp16x3 path: device scalars >= max|A operand| and max|weights| (null on the other paths)
    const float* a_bound; const float* w_bound;
    int N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil;
    int M, K, mtiles, ntiles;
    // optional (conv3s.hip MODE 4, data-gradient launches with the BatchNorm-backward epilogue): the A operand is formed while it is
    // staged as  scale (x - c0 - (ap_y - mean) invstd c1)  — x = dL/dz of the BatchNorm behind this convolution, ap_y its input,
    // ap_coef = [c0 | c1] — and the patch's own pixels of it are written to ap_out (the materialised dL/dy)
    const float* ap_y; const float* ap_scale; const float* ap_mean; const float* ap_invstd; const float* ap_coef; float* ap_out;
    // optional: the operand bounds this launch leaves for the consumers of its output (bn_pro.h)
    OutBoundsP tail;
    // optional (pro.partial != null): the BatchNorm of the A operand is finalised in this launch's prologue — every
    // workgroup writes in_scale / in_shift (= pro.scale / pro.shift) itself before it reads them (bn_pro.h)
    BnProP pro;
};

// ---- host side
// the twelve geometry fields and the GEMM sizes M, K of a kernel-argument struct (ConvP, WgradP)
template <class P>
static inline void conv_geom_fill(P& p, const dsnt_conv_geom* g) {
    p.N = g->N; p.H = g->H; p.W = g->W; p.Cin = g->Cin; p.Ho = g->Ho; p.Wo = g->Wo;
    p.Cout = g->Cout; p.R = g->R; p.S = g->S; p.stride = g->stride; p.pad = g->pad; p.dil = g->dil;
    p.M = g->N * g->Ho * g->Wo; p.K = g->R * g->S * g->Cin;
}
// geometry checks of every convolution entry point; `who` names the caller in the message (conv_f32.hip)
int conv_check_geom(const dsnt_conv_geom* g, const char* who);
// Checks the arguments of a forward / data-gradient launch and fills `p` with everything but the tile counts and the BatchNorm
// prologue (zeroed).  planes: `w` holds split weight planes `plane_stride` elements apart (p.wq) instead of fp32 weights (p.w),
// and the geometry has to pass dsnt_conv_bf16x6_ok.  Messages name `who`, those about bnb / tail `who`_ex.  (conv_f32.hip)
int conv_fill(ConvP& p, const char* who, const float* x, const void* w, bool planes, int64_t plane_stride, const float* bias,
              float* y, const float* in_scale, const float* in_shift, int in_relu, const float* res1, const float* res2,
              float* stats_partial, const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail);
