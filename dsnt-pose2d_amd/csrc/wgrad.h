// Internal interface of the weight-gradient kernel units behind the dispatch in conv_wgrad.hip: a plan and a launch for the halo
// kernels (wgrad3.hip), the 1x1 kernels (wgrad1.hip) and the implicit GEMMs (wgrad_gemm.hip), and the slab reduction
// (wgrad_reduce.hip) that follows any of them.  (The stem's kernel: stem4.h.)
#pragma once
#include "common.h"

// ---- 3x3 / stride 1 weight gradients (wgrad3.hip)
// Plan of one launch: which instantiation, how the pixels are cut into slabs.  ok == 0: geometry not supported.
struct Wg3Plan {
    int ok;
    int cfg;            // 0: 64 x 128 channels per workgroup (9 taps per wave), 1: 64 x 64 (taps split over two wave
                        // groups); a cfg-0 launch that SHARES the chip runs as 32 x 128 four-wave workgroups instead
                        // (same slabs: twice the channel chunks)
    int WS;             // strip width in pixels (16, 32 or 64)
    int strips;         // W / WS
    int rps;            // output rows per slab (divides H)
    int hsplits;        // H / rps
    int kchunks;        // Cin / 64
    int nchunks;        // Cout / (128 or 64)
    int nslabs;         // N * hsplits * strips: slabs ws[nslabs][Cout][K] (+ [nslabs][Cout] bias partials)
    int blocks;         // workgroups
    int lds;            // dynamic LDS bytes
};
// share = DSNT_WGRAD_SHARE_CHIP: the plan of a launch that runs beside a dependency chain (fewer, longer slabs)
Wg3Plan dsnt_wg3_plan(const dsnt_conv_geom* g, int share);      // share: 0 whole chip, 1 beside a chain, 2 the same, narrower
// enqueue (or record) the launch; tensors as dsnt_conv_wgrad_f16x3 (in_scale / in_shift may be null); share =
// DSNT_WGRAD_SHARE_CHIP: the launch runs beside a dependency chain on another stream
void dsnt_wg3_launch(const Wg3Plan& pl, const float* x, const float* in_scale, const float* in_shift, int in_relu,
                     const float* dy, float* ws, const float* a_bound, const float* g_bound, const dsnt_conv_geom* g,
                     hipStream_t st, int share);

// ---- 1x1 weight gradients (wgrad1.hip): a four-wave workgroup owns ck x cn channels of the weight matrix for its pixels
struct Wg1Plan {
    int ok;
    int ck, cn;             // input / output channels per workgroup (64, 128 or 256)
    int kchunks, nchunks;   // Cin / ck, Cout / cn
    int nsplits;            // slabs ws[nsplits][Cout][Cin] (+ [nsplits][Cout] bias partials)
    int rows_per_split;     // multiple of 16
    int blocks, lds;
};
Wg1Plan dsnt_wg1_plan(const dsnt_conv_geom* g, bool share);
void dsnt_wg1_launch(const Wg1Plan& pl, const float* x, const float* in_scale, const float* in_shift, int in_relu,
                     const float* dy, float* ws, const float* a_bound, const float* g_bound, const dsnt_conv_geom* g,
                     hipStream_t st);

// ---- implicit-GEMM weight gradients (wgrad_gemm.hip): every geometry, 128 x 128 tiles of the weight matrix per workgroup
struct WgGemmPlan {
    int ktiles, ntiles;     // ceil(K / 128), ceil(Cout / 128)
    int splits;             // slabs ws[splits][Cout][K] (+ [splits][Cout] bias partials); 0: a geometry without pixels or weights
    int rows_per_split;     // multiple of 32
};
WgGemmPlan dsnt_wgg_plan(const dsnt_conv_geom* g);
// bf16x6 = false: the fp32-MFMA kernel; true: the role-split kernel, fp16x3 where both bounds are given, else bf16x6.
// share = DSNT_WGRAD_SHARE_CHIP (role-split kernel only): one workgroup per CU
void dsnt_wgg_launch(const WgGemmPlan& pl, bool bf16x6, const float* x, const float* in_scale, const float* in_shift,
                     int in_relu, const float* dy, float* ws, const float* a_bound, const float* g_bound,
                     const dsnt_conv_geom* g, hipStream_t st, bool share);
// the grouped launch: one row of dsnt_wgg_desc_bytes() bytes per convolution, filled by dsnt_wgg_desc (bounds null: bf16x6),
// which returns the row's workgroups
int dsnt_wgg_desc_bytes(void);
int dsnt_wgg_desc(const float* x, const float* in_scale, const float* in_shift, int in_relu, const float* dy, float* ws,
                  const float* a_bound, const float* g_bound, const dsnt_conv_geom* g, void* desc_out);
void dsnt_wgg_launch_group(const void* table, int nconv, int max_blocks, hipStream_t st);

// ---- slab reduction (wgrad_reduce.hip): dw[Cout][K] (+ dbias[Cout], may be null) from `slabs` slabs of any kernel above;
// CK = Cout * K, accumulate = 0 / 1
void wgrad_reduce_launch(const float* ws, float* dw, float* dbias, int slabs, int CK, int Cout, int accumulate,
                         hipStream_t st);

// ---- the dispatch (conv_wgrad.hip): dsnt_conv_f16x3_route(g, 1) for a geometry conv_check_geom accepts
int dsnt_wgrad_route_kind(const dsnt_conv_geom* g);
