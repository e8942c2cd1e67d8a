// What the two kernels of the symmetric 3x3 convolution share — conv3s.hip (v_mfma_f32_32x32x16_f16) and conv3s_mf.hip
// (v_mfma_f32_16x16x32_f16): the pieces that do not depend on the MFMA form.  Each kernel owns its LDS layout, its weight ring, its
// fragment schedule and its epilogue's register layout; an LDS destination is always computed by the caller.
#pragma once
#include "conv3s.h"

typedef unsigned c3_u32x4 __attribute__((ext_vector_type(4)));
typedef float c3_f32x4 __attribute__((ext_vector_type(4)));
typedef int c3_i32x4 __attribute__((ext_vector_type(4)));

#define C3_OOB 0xF0000000u                  /* a buffer offset behind every resource: the load returns zeros, the store is dropped */

// A tile is a patch of 128 / PW rows x PW output pixels — 4 x 32 (W % 32 == 0), or 8 x 16 for the 16-pixel-wide levels — x all
// columns; its input is the (PH + 2) x (PW + 2) halo.  Halo staging works in items: item j (0..3) of a thread = halo pixel
// (tid >> 2) + 64 j, 4-channel quad tid & 3 of a 16-channel chunk.
template <int PW> struct C3Patch {
    static constexpr int PH = 128 / PW, HW = PW + 2, HPX = (PH + 2) * HW, ITEMS = HPX * 4;
};

// Global byte offsets (aoffs) of the thread's four halo items in the tile with virtual index vv (xcd_remap gives the tile; beyond
// ntiles: nothing is live) and their flags — bits 0-3: the halo pixel of item j lies inside the image; bits 4-7 (OWN: the folded
// BatchNorm backward): it is one of the patch's own pixels.  tws x ths patches per image.  Returns the tile's first output pixel.
template <int PW, bool OWN>
__device__ __forceinline__ int c3_set_tile(const ConvP& p, const int& ntiles, const int& tws, const int& ths, const int vv, const int& tid,
                                           const int& kc, unsigned (&aoffs)[4], unsigned& aokn) {
    typedef C3Patch<PW> T;
    aokn = 0;
    int img = 0, th = 0, tw = 0;
    const bool live = vv < ntiles;
    if (live) {
        int tile;
        xcd_remap(vv, ntiles, tile);
        tw = tile % tws;
        th = (tile / tws) % ths;
        img = tile / (tws * ths);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int px = (tid >> 2) + 64 * j;
        const int hy = px / T::HW, hx = px - hy * T::HW;
        const int ih = th * T::PH - 1 + hy, iw = tw * PW - 1 + hx;
        const bool in = live && px < T::HPX && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        aoffs[j] = in ? (unsigned)(((img * p.H + ih) * p.W + iw) * p.Cin + kc * 4) * 4u : C3_OOB;
        aokn |= (in ? 1u : 0u) << j;
        if (OWN) aokn |= ((in && hy >= 1 && hy <= T::PH && hx >= 1 && hx <= PW) ? 16u : 0u) << j;
    }
    return (img * p.H + th * T::PH) * p.W + tw * PW;
}

// The vectors of the operand transform in LDS (SS): PRO — [2][Cin] BatchNorm scale / shift, the operand scale sa riding in them;
// APPLY — [3][Cin] P, R, S of  dy = scale (dz - c0 - (y - mean) invstd c1) = P dz + R y + S.
template <bool PRO, bool APPLY>
__device__ __forceinline__ void c3_fill_vectors(const ConvP& p, float* const& SS, const float& sa, const int& tid) {
    if (APPLY) {
        for (int k = tid; k < p.Cin; k += 256) {
            const float sc = p.ap_scale[k], is = p.ap_invstd[k], mu = p.ap_mean[k], c0 = p.ap_coef[k], c1 = p.ap_coef[p.Cin + k];
            const float q = sc * is * c1;
            SS[k] = sc;                                             // dy = P dz + (S - Q y)
            SS[p.Cin + k] = -q;
            SS[2 * p.Cin + k] = (float)((double)q * (double)mu - (double)sc * (double)c0);
        }
        __syncthreads();
    }
    if (PRO) {
        for (int k = tid; k < p.Cin; k += 256) {
            SS[k] = p.in_scale[k] * sa;
            SS[p.Cin + k] = p.in_shift[k] * sa;
        }
        __syncthreads();
    }
}

// Item j of chunk c (channels 4 kc .. 4 kc + 3; okb: the flags of its tile, aoff: its global offset): transform — the BatchNorm +
// ReLU prologue (PRO), the folded BatchNorm backward (APPLY: a = dL/dz, b = y; the formed dL/dy of a pixel of the patch's own also
// goes to `dor`) or the operand scale alone — and the fp16 hi / lo split.
// NO branch on the thread index in here: a divergent branch costs nothing by itself, but it ends the basic block, and the ~50 VALU
// instructions of an item then cannot be scheduled between the MFMAs of the step — they run as one clump with the matrix pipe idle
// on both waves of the SIMD.
// (References, here and in c3_set_tile: the callers' locals as their own lambdas would capture them.)
template <bool PRO, bool APPLY>
__device__ __forceinline__ void c3_item(const ConvP& p, float* const& SS, const c3_u32x4 a, const c3_u32x4 b, const int c, const int j,
                                        const unsigned okb, const int& kc, const float& lo_valid, const float& sa,
                                        const __amdgpu_buffer_rsrc_t& dor, const unsigned& aoff, uint2& q1, uint2& q2) {
    float4 v = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
    if (PRO) {
        const float4 sc = *reinterpret_cast<const float4*>(SS + c * 16 + kc * 4);
        const float4 sh = *reinterpret_cast<const float4*>(SS + p.Cin + c * 16 + kc * 4);
        // BN FMAs; ReLU + zero padding (applied after BN + ReLU) as one median per element
        const bool ok = (okb >> j) & 1u;
        const float lo = ok ? lo_valid : 0.f, hi = ok ? __builtin_inff() : 0.f;
        v.x = __builtin_amdgcn_fmed3f(fmaf(v.x, sc.x, sh.x), lo, hi);
        v.y = __builtin_amdgcn_fmed3f(fmaf(v.y, sc.y, sh.y), lo, hi);
        v.z = __builtin_amdgcn_fmed3f(fmaf(v.z, sc.z, sh.z), lo, hi);
        v.w = __builtin_amdgcn_fmed3f(fmaf(v.w, sc.w, sh.w), lo, hi);
    } else if (APPLY) {
        const float4 sc = *reinterpret_cast<const float4*>(SS + c * 16 + kc * 4);
        const float4 sh = *reinterpret_cast<const float4*>(SS + p.Cin + c * 16 + kc * 4);
        const float4 sq = *reinterpret_cast<const float4*>(SS + 2 * p.Cin + c * 16 + kc * 4);
        // dy = P dz + (R y + S); a pixel outside the image is zero padding of dy (both loads returned zeros: mask S)
        const bool ok = (okb >> j) & 1u;
        v.x = fmaf(v.x, sc.x, fmaf(__uint_as_float(b.x), sh.x, ok ? sq.x : 0.f));
        v.y = fmaf(v.y, sc.y, fmaf(__uint_as_float(b.y), sh.y, ok ? sq.y : 0.f));
        v.z = fmaf(v.z, sc.z, fmaf(__uint_as_float(b.z), sh.z, ok ? sq.z : 0.f));
        v.w = fmaf(v.w, sc.w, fmaf(__uint_as_float(b.w), sh.w, ok ? sq.w : 0.f));
        // (no branch: a pixel of the halo ring gets an out-of-range offset and the store is dropped)
        __builtin_amdgcn_raw_buffer_store_b128((c3_u32x4){__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z),
                                                          __float_as_uint(v.w)}, dor, ((okb >> (4 + j)) & 1u) ? aoff : C3_OOB, c * 64, 0);
        v.x *= sa; v.y *= sa; v.z *= sa; v.w *= sa;
    } else {
        v.x *= sa; v.y *= sa; v.z *= sa; v.w *= sa;
    }
    split4h(v, q1, q2);
}

// per-column vectors of the epilogue: the BatchNorm backward's (BNB), or the bias and the vectors of the BatchNorm + ReLU bound
struct C3Col { float cb, sc, sh, mu, is; };
template <bool BNB>
__device__ __forceinline__ C3Col c3_loadcol(const ConvP& p, const int n) {
    C3Col c = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (BNB) { c.sc = p.bnb_scale[n]; c.sh = p.bnb_shift[n]; c.mu = p.bnb_mean[n]; c.is = p.bnb_invstd[n]; }
    else {
        if (p.bias) c.cb = p.bias[n];
        if (p.tail.amax_bn) { c.sc = p.tail.amax_scale[n]; c.sh = p.tail.amax_shift[n]; }
    }
    return c;
}

// per-tile column statistics: the WM row groups' partial sums red[WM][CO][2] (written by the epilogue) -> p.stats[tile][2][Cout]
template <int CO, int WM>
__device__ __forceinline__ void c3_tile_stats(const ConvP& p, float* const& red, const int& v, const int& ntiles, const int& choff,
                                              const int& tid) {
    int tile;
    xcd_remap(v, ntiles, tile);
    __syncthreads();
    for (int u = tid; u < CO * 2; u += 256) {
        const int which = u & 1, c = u >> 1;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) s += red[(w * CO + c) * 2 + which];
        tail_store(p.stats + ((size_t)tile * 2 + which) * p.Cout + choff + c, s);
    }
    __syncthreads();                    // `red` is written again (32x32x16: the next weight pair is stored over it)
}

// the 16x16x32 kernel's launch (conv3s_mf.hip): Cout 128 forward on 4 x 32 patches, on `grid` persistent workgroups; c3_form in
// conv3s.hip decides that a launch goes here
void dsnt_conv3s_mf_launch(const ConvP& p, bool pro, hipStream_t st, int grid, int ntiles);
