// The dsnt_conv_wgrad* entry points: host code only.  One route (which kernel unit takes a geometry, its plan, how many slabs),
// one argument check and one launch path for all of them, and the workspace, slab-count and descriptor queries answered from
// the same route.  The kernels: stem4.hip, wgrad3.hip, wgrad1.hip and wgrad_gemm.hip behind stem4.h / wgrad.h; the slab
// reduction: wgrad_reduce.hip.
#include "conv_split.h"
#include "wgrad.h"
#include "stem4.h"
#include <string.h>

// ---- the route.  The kinds are the values of dsnt_conv_f16x3_route(g, 1).
enum { WG_GEMM = 0, WG_STEM = 1, WG_HALO = 2, WG_ONE = 3 };
struct WgradRoute {
    int kind;
    int slabs;              // ws[slabs][Cout][K] (+ [slabs][Cout] bias partials)
    int K;                  // R * S * Cin
    int share;              // WG_HALO: the `share` argument its plan was made with, and its launch takes
    Wg3Plan halo;           // the plan of `kind` (the stem kernel has none beyond its slabs); the others are zero
    Wg1Plan one;
    WgGemmPlan gemm;
};

static WgradRoute wgrad_route_gemm(const dsnt_conv_geom* g) {
    WgradRoute r;
    memset(&r, 0, sizeof(r));
    r.kind = WG_GEMM;
    r.K = g->R * g->S * g->Cin;
    r.gemm = dsnt_wgg_plan(g);
    r.slabs = r.gemm.splits;
    return r;
}

// Where dsnt_conv_wgrad_f16x3 takes geometry g with these `accumulate` flags: stem -> halo -> 1x1 -> implicit GEMM, the first
// whose plan accepts it.  The launch, the slab / workspace queries and the route query all ask here, so a workspace is sized
// for the kernel that then writes it.
static WgradRoute wgrad_route(const dsnt_conv_geom* g, int accumulate) {
    WgradRoute r;
    memset(&r, 0, sizeof(r));
    r.K = g->R * g->S * g->Cin;
    // the stem's space-to-depth convolution (4x4, 16 -> 64 channels, raw operand): its own kernel (stem4.hip), one slab per workgroup
    if (const int s4 = dsnt_stem4_wgrad_slabs(g)) {
        r.kind = WG_STEM; r.slabs = s4;
        return r;
    }
    // 3x3 / stride 1 convolutions: the halo kernel (wgrad3.hip) — every operand element staged once for all nine taps.
    // `accumulate` flags -> its plan: 0 whole chip, 1 DSNT_WGRAD_SHARE_CHIP, 2 with DSNT_WGRAD_NARROW on top
    const bool share = (accumulate & DSNT_WGRAD_SHARE_CHIP) != 0;
    r.share = share ? ((accumulate & DSNT_WGRAD_NARROW) ? 2 : 1) : 0;
    r.halo = dsnt_wg3_plan(g, r.share);
    if (r.halo.ok) {
        r.kind = WG_HALO; r.slabs = r.halo.nslabs;
        return r;
    }
    // 1x1 convolutions of >= 16384 rows: the transposition-free four-wave kernel (wgrad1.hip)
    r.one = dsnt_wg1_plan(g, share);
    if (r.one.ok) {
        r.kind = WG_ONE; r.slabs = r.one.nsplits;
        return r;
    }
    return wgrad_route_gemm(g);
}

// floats of a workspace of `slabs` slabs: the slabs, then the bias partials
static int64_t wgrad_slab_floats(int64_t slabs, const dsnt_conv_geom* g) {
    return slabs * ((int64_t)g->Cout * (g->R * g->S * g->Cin) + g->Cout);
}

// ---- the check and the launch
struct WgradArgs {
    const float* x; const float* in_scale; const float* in_shift; int in_relu;
    const float* dy; float* ws; float* dw; float* dbias; int accumulate;
    const float* a_bound; const float* g_bound;       // fp16x3; null otherwise
};

// (the implicit GEMM reports as dsnt_conv_wgrad whichever entry point reached it: the texts are part of the ABI)
static const char* wgrad_who(int kind) { return kind == WG_GEMM ? "dsnt_conv_wgrad" : "dsnt_conv_wgrad_f16x3"; }

// The order of the checks is part of the ABI (callers see the first failure): geometry, null tensor, dbias without dw, the
// scale / shift pair (raw: the stem kernel has no BatchNorm prologue), alignment.
static int wgrad_check(const char* who, bool raw, const WgradArgs& a, const dsnt_conv_geom* g) {
    if (int e = conv_check_geom(g, who)) return e;
    DSNT_REQUIRE(a.x && a.dy && a.ws, DSNT_ERR_ARG, "%s: null tensor", who);
    DSNT_REQUIRE(a.dw || !a.dbias, DSNT_ERR_ARG, "%s: dbias without dw", who);
    if (raw)
        DSNT_REQUIRE(!a.in_scale && !a.in_shift, DSNT_ERR_ARG, "%s: the 4x4 / 16 -> 64 stem geometry takes a raw operand only", who);
    else
        DSNT_REQUIRE((a.in_scale == nullptr) == (a.in_shift == nullptr), DSNT_ERR_ARG, "%s: in_scale/in_shift must be given together", who);
    DSNT_REQUIRE(dsnt_aligned16(a.x) && dsnt_aligned16(a.dy) && dsnt_aligned16(a.ws) && (!a.dw || dsnt_aligned16(a.dw)),
                 DSNT_ERR_ALIGN, "%s: tensors must be 16-byte aligned", who);
    return DSNT_OK;
}

// The kernel of the route, then the reduction of its slabs unless the caller reduces later (dw == nullptr: slabs only,
// dsnt_wgrad_reduce_all).  bf16x6: the WG_GEMM kernel family (see dsnt_wgg_launch).
static int wgrad_launch(const WgradRoute& r, bool bf16x6, const WgradArgs& a, const dsnt_conv_geom* g, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    switch (r.kind) {
    case WG_STEM:
        dsnt_stem4_wgrad_launch(a.x, a.dy, a.ws, a.a_bound, a.g_bound, g, st);
        break;
    case WG_HALO:
        dsnt_wg3_launch(r.halo, a.x, a.in_scale, a.in_shift, a.in_relu, a.dy, a.ws, a.a_bound, a.g_bound, g, st, r.share);
        break;
    case WG_ONE:
        dsnt_wg1_launch(r.one, a.x, a.in_scale, a.in_shift, a.in_relu, a.dy, a.ws, a.a_bound, a.g_bound, g, st);
        break;
    default:
        dsnt_wgg_launch(r.gemm, bf16x6, a.x, a.in_scale, a.in_shift, a.in_relu, a.dy, a.ws, a.a_bound, a.g_bound, g, st,
                        (a.accumulate & DSNT_WGRAD_SHARE_CHIP) != 0);
    }
    if (a.dw) wgrad_reduce_launch(a.ws, a.dw, a.dbias, r.slabs, g->Cout * r.K, g->Cout, a.accumulate & 1, st);
    DSNT_CHECK_LAUNCH(wgrad_who(r.kind));
}

// ---- entry points
extern "C" int dsnt_conv_wgrad(const float* x, const float* in_scale, const float* in_shift,
                               int in_relu, const float* dy, float* ws, float* dw, float* dbias,
                               int accumulate, const dsnt_conv_geom* g, void* stream) {
    const WgradArgs a = {x, in_scale, in_shift, in_relu, dy, ws, dw, dbias, accumulate, nullptr, nullptr};
    if (int e = wgrad_check(wgrad_who(WG_GEMM), false, a, g)) return e;
    return wgrad_launch(wgrad_route_gemm(g), false, a, g, stream);
}

extern "C" int dsnt_conv_wgrad_bf16x6_ok(const dsnt_conv_geom* g) {
    if (!g) return 0;
    return g->Cin % 4 == 0 && g->Cout % 4 == 0 && g->Wo % 4 == 0 &&
           (size_t)g->N * g->H * g->W * g->Cin * 4u < (1ull << 31) &&
           (size_t)g->N * g->Ho * g->Wo * g->Cout * 4u < (1ull << 31);
}

extern "C" int dsnt_conv_wgrad_bf16x6(const float* x, const float* in_scale, const float* in_shift,
                                      int in_relu, const float* dy, float* ws, float* dw, float* dbias,
                                      int accumulate, const dsnt_conv_geom* g, void* stream) {
    DSNT_REQUIRE(dsnt_conv_wgrad_bf16x6_ok(g), DSNT_ERR_SHAPE,
                 "dsnt_conv_wgrad_bf16x6: geometry not supported (need Wo %% 4 == 0, tensors < 2 GiB)");
    const WgradArgs a = {x, in_scale, in_shift, in_relu, dy, ws, dw, dbias, accumulate, nullptr, nullptr};
    if (int e = wgrad_check(wgrad_who(WG_GEMM), false, a, g)) return e;
    return wgrad_launch(wgrad_route_gemm(g), true, a, g, stream);
}

extern "C" int dsnt_conv_wgrad_f16x3(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                                     const float* dy, float* ws, float* dw, float* dbias, int accumulate,
                                     const float* a_bound, const float* g_bound, const dsnt_conv_geom* g, void* stream) {
    DSNT_REQUIRE(dsnt_conv_wgrad_bf16x6_ok(g), DSNT_ERR_SHAPE,
                 "dsnt_conv_wgrad_f16x3: geometry not supported (need Wo %% 4 == 0, tensors < 2 GiB)");
    DSNT_REQUIRE(a_bound && g_bound, DSNT_ERR_ARG, "dsnt_conv_wgrad_f16x3: both operand bounds are required");
    const WgradArgs a = {x, in_scale, in_shift, in_relu, dy, ws, dw, dbias, accumulate, a_bound, g_bound};
    const WgradRoute r = wgrad_route(g, accumulate);
    if (int e = wgrad_check(wgrad_who(r.kind), r.kind == WG_STEM, a, g)) return e;
    return wgrad_launch(r, true, a, g, stream);
}

// ---- queries
// Plan of dsnt_conv_wgrad / dsnt_conv_wgrad_bf16x6 (always the implicit GEMM): number of slabs to reduce
extern "C" int dsnt_conv_wgrad_splits(const dsnt_conv_geom* g) { return g ? wgrad_route_gemm(g).slabs : 0; }

// Plan of dsnt_conv_wgrad_f16x3: number of slabs to reduce and workspace floats for a launch with these `accumulate` flags
// (DSNT_WGRAD_SHARE_CHIP / DSNT_WGRAD_NARROW change the halo and 1x1 kernels' plans); equal to dsnt_conv_wgrad_splits and that
// many slabs where the implicit-GEMM kernel runs.
extern "C" int dsnt_conv_wgrad_f16x3_splits(const dsnt_conv_geom* g, int accumulate) {
    return g ? wgrad_route(g, accumulate).slabs : 0;
}
extern "C" int64_t dsnt_conv_wgrad_f16x3_ws_floats(const dsnt_conv_geom* g, int accumulate) {
    return g ? wgrad_slab_floats(wgrad_route(g, accumulate).slabs, g) : 0;
}
// Enough for ANY of the weight-gradient entry points on this geometry, with or without DSNT_WGRAD_SHARE_CHIP (the stem, halo
// and 1x1 kernels cut the pixels into their own, sometimes more, slabs: dsnt_conv_wgrad_f16x3_ws_floats is the exact size of
// that call; DSNT_WGRAD_NARROW only ever halves the slabs)
extern "C" int64_t dsnt_conv_wgrad_ws_floats(const dsnt_conv_geom* g) {
    if (!g) return 0;
    int slabs = wgrad_route_gemm(g).slabs;
    for (const int accumulate : {0, DSNT_WGRAD_SHARE_CHIP}) {
        const int s = wgrad_route(g, accumulate).slabs;
        if (s > slabs) slabs = s;
    }
    return wgrad_slab_floats(slabs, g);
}
extern "C" int dsnt_conv_wgrad_halo_ok(const dsnt_conv_geom* g) { return g && wgrad_route(g, 0).kind == WG_HALO; }
// dsnt_conv_f16x3_route(g, 1) (conv_split6.hip) behind its geometry check
int dsnt_wgrad_route_kind(const dsnt_conv_geom* g) { return dsnt_conv_wgrad_bf16x6_ok(g) ? wgrad_route(g, 0).kind : -1; }

// ---- the grouped launch and its descriptors (wgrad_gemm.hip)
extern "C" int dsnt_conv_wgrad_desc_bytes(void) { return dsnt_wgg_desc_bytes(); }

// both descriptor entry points; bounds: the fp16x3 one, which needs a_bound and g_bound.  Returns the workgroups or -(error code)
static int wgrad_desc(const char* who, bool bounds, const float* x, const float* in_scale, const float* in_shift, int in_relu,
                      const float* dy, float* ws, const float* a_bound, const float* g_bound, const dsnt_conv_geom* g,
                      void* desc_out) {
    if (int e = conv_check_geom(g, who)) return -e;
    if (!x || !dy || !ws || !in_scale || !in_shift || !desc_out || (bounds && (!a_bound || !g_bound)) ||
        !dsnt_conv_wgrad_bf16x6_ok(g) || !dsnt_aligned16(x) || !dsnt_aligned16(dy) || !dsnt_aligned16(ws)) {
        return -dsnt_set_error(DSNT_ERR_ARG, "%s: needs x, dy, ws (16-byte aligned), in_scale/in_shift%s a geometry "
                                             "dsnt_conv_wgrad_bf16x6_ok accepts", who, bounds ? ", both operand bounds and" : " and");
    }
    return dsnt_wgg_desc(x, in_scale, in_shift, in_relu, dy, ws, a_bound, g_bound, g, desc_out);
}
extern "C" int dsnt_conv_wgrad_desc(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                                    const float* dy, float* ws, const dsnt_conv_geom* g, void* desc_out) {
    return wgrad_desc("dsnt_conv_wgrad_desc", false, x, in_scale, in_shift, in_relu, dy, ws, nullptr, nullptr, g, desc_out);
}
extern "C" int dsnt_conv_wgrad_desc_f16x3(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                                          const float* dy, float* ws, const float* a_bound, const float* g_bound,
                                          const dsnt_conv_geom* g, void* desc_out) {
    return wgrad_desc("dsnt_conv_wgrad_desc_f16x3", true, x, in_scale, in_shift, in_relu, dy, ws, a_bound, g_bound, g, desc_out);
}

extern "C" int dsnt_conv_wgrad_group(const void* table, int nconv, int max_blocks, void* stream) {
    DSNT_REQUIRE(table && nconv > 0 && nconv <= 65535 && max_blocks > 0, DSNT_ERR_ARG,
                 "dsnt_conv_wgrad_group: bad argument");
    dsnt_wgg_launch_group(table, nconv, max_blocks, (hipStream_t)stream);
    DSNT_CHECK_LAUNCH("dsnt_conv_wgrad_group");
}
