// dsnt_render_pose: skeleton and heat-map overlays of a batch in one launch (contract: include/dsnt_hip.h, DESIGN.md
// section 15).  A gather: every thread owns RENDER_PX consecutive pixels of one row and writes their bytes once.
//
// Workgroup (tile, b) owns a RENDER_TW x RENDER_TH tile of sample b.  Wave 0 first maps the sample's joints to continuous
// pixel units in LDS, then tests every bone's (and disc's) bounding box, grown by the coverage radius, against the tile;
// the two ballots are the tile's work list, so a tile away from the skeleton does no segment work and bones keep their
// table order.  The bone and colour tables are host arrays that travel in the kernel arguments, so a call copies nothing
// to the device; wave 0 copies them to LDS with one lane per entry and every later read is an LDS broadcast.  Built with -ffp-contract=off: the canvas steps are rounded one by one, as torch rounds them.
#include "common.h"
#include <math.h>

namespace {

constexpr int RENDER_NT = 256;
constexpr int RENDER_PX = 4;                 // 4 RGB pixels = 12 bytes = 3 dwords per thread
constexpr int RENDER_TW = 64;                // tile: 16 threads x 4 pixels wide (192 contiguous bytes per row) ...
constexpr int RENDER_TH = RENDER_NT / (RENDER_TW / RENDER_PX);      // ... and 16 rows high
static_assert(DSNT_RENDER_MAX_JOINTS == DSNT_WAVE, "one lane of wave 0 per joint, one ballot for the discs");
static_assert(DSNT_RENDER_MAX_BONES <= 32, "the tile's bones are one 32-bit mask");

struct RenderParams {
    const void* canvas;                      // f32 [B][3][H][W], uint8 [B][H][W][3] or unused
    const float* hm;                         // f32 [B][J][h][w] or NULL
    const float* peak;                       // element (b, j) at peak[(b * J + j) * peak_stride]
    const float* coords;                     // f32 [B][J][2]
    const float* mask;                       // f32 [B][J] or NULL
    uint8_t* out;                            // uint8 [B][H][W][3]
    int64_t peak_stride;
    int kind, H, W, J, h, w, nheat, nbones, pixel_coords, tiles_x;
    float mean[3], stdv[3];
    float heat_alpha, reach, disc_reach;     // reach = width / 2 + 0.5; disc_reach = joint_radius + 0.5, or 0: no discs
    unsigned char heat_joint[DSNT_RENDER_MAX_JOINTS];            // the nheat joints whose colour is not black, ascending
    float heat_rgb[DSNT_RENDER_MAX_JOINTS][3];                   // their colours, [0, 1]
    unsigned char bone_j1[DSNT_RENDER_MAX_BONES], bone_j2[DSNT_RENDER_MAX_BONES];
    float bone_rgb[DSNT_RENDER_MAX_BONES][3];                    // 0..255
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }          // NaN -> 0

// value = value * (1 - cov) + rgb * cov with cov = clamp(reach - d, 0, 1), d the distance of (cx, cy) to the segment
// p + t e, t in [0, 1] (inv_ee = 1 / |e|^2, or 0 for a point)
__device__ __forceinline__ void cover(float (&val)[3], float cx, float cy, float px, float py, float ex, float ey,
                                      float inv_ee, float reach, float r, float g, float b) {
    const float qx = cx - px, qy = cy - py;
    const float t = clamp01((qx * ex + qy * ey) * inv_ee);
    const float dx = qx - t * ex, dy = qy - t * ey;
    const float cov = clamp01(reach - sqrtf(dx * dx + dy * dy));
    val[0] = val[0] * (1.f - cov) + r * cov;
    val[1] = val[1] * (1.f - cov) + g * cov;
    val[2] = val[2] * (1.f - cov) + b * cov;
}

__global__ void __launch_bounds__(RENDER_NT) render_pose_kernel(const RenderParams p) {
    __shared__ float ju[DSNT_RENDER_MAX_JOINTS], jv[DSNT_RENDER_MAX_JOINTS];
    __shared__ int jstate[DSNT_RENDER_MAX_JOINTS];       // bit 0: finite, bit 1: masked out, bits 8..: colour bone + 1 (0: none)
    // the tables of the argument block, copied by wave 0 with one lane per entry.  Do not index the argument block itself
    // with the (uniform) bone number instead: built that way, bones k % 4 != 0 came out on the MI355X in the colour
    // components one float earlier, which the golden-skeleton test shows as blue bones drawn red
    __shared__ int bone_j[DSNT_RENDER_MAX_BONES];        // j1 | j2 << 8
    __shared__ float bone_c[DSNT_RENDER_MAX_BONES][3];
    __shared__ int heat_j[DSNT_RENDER_MAX_JOINTS];
    __shared__ float heat_c[DSNT_RENDER_MAX_JOINTS][3];
    __shared__ unsigned tile_bones;
    __shared__ unsigned long long tile_discs;
    const int b = blockIdx.y;
    const int tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int x0t = tile_x * RENDER_TW, y0t = tile_y * RENDER_TH;
    const int t = threadIdx.x;
    const int H = p.H, W = p.W, J = p.J;

    if (p.nbones > 0 || p.nheat > 0) {
        if (t < DSNT_WAVE) {
            if (t < p.nheat) {
                heat_j[t] = p.heat_joint[t];
                for (int c = 0; c < 3; ++c) heat_c[t][c] = p.heat_rgb[t][c];
            }
            if (t < p.nbones) {
                bone_j[t] = p.bone_j1[t] | (p.bone_j2[t] << 8);
                for (int c = 0; c < 3; ++c) bone_c[t][c] = p.bone_rgb[t][c];
            }
            float u = 0.f, v = 0.f;
            int st = 0;
            if (p.nbones > 0 && t < J) {
                u = p.coords[((size_t)b * J + t) * 2];
                v = p.coords[((size_t)b * J + t) * 2 + 1];
                if (!p.pixel_coords) {
                    u = (u + 1.f) * (0.5f * (float)W);
                    v = (v + 1.f) * (0.5f * (float)H);
                }
                if (isfinite(u) && isfinite(v)) st |= 1;
                if (p.mask && p.mask[(size_t)b * J + t] == 0.f) st |= 2;
            }
            ju[t] = u;
            jv[t] = v;
            jstate[t] = st;
        }
        __syncthreads();
        if (p.nbones > 0 && t < DSNT_WAVE) {
            const float tx0 = (float)x0t, tx1 = (float)(x0t + RENDER_TW), ty0 = (float)y0t, ty1 = (float)(y0t + RENDER_TH);
            bool hit = false;
            if (t < p.nbones) {
                const int j1 = bone_j[t] & 0xff, j2 = bone_j[t] >> 8;
                if (jstate[j1] & jstate[j2] & 1) {
                    const float r = p.reach;
                    hit = fmaxf(ju[j1], ju[j2]) + r >= tx0 && fminf(ju[j1], ju[j2]) - r <= tx1 &&
                          fmaxf(jv[j1], jv[j2]) + r >= ty0 && fminf(jv[j1], jv[j2]) - r <= ty1;
                }
            }
            const unsigned long long bones = __ballot(hit);
            int st = jstate[t];
            bool disc = false;
            if (p.disc_reach > 0.f && t < J && (st & 1)) {
                int first = 0;                                       // the first bone of the table that names the joint, + 1
                for (int k = p.nbones - 1; k >= 0; --k)
                    if ((bone_j[k] & 0xff) == t || (bone_j[k] >> 8) == t) first = k + 1;
                st |= first << 8;
                if (first) {
                    const float r = p.disc_reach;
                    disc = ju[t] + r >= tx0 && ju[t] - r <= tx1 && jv[t] + r >= ty0 && jv[t] - r <= ty1;
                }
            }
            const unsigned long long discs = __ballot(disc);
            jstate[t] = st;
            if (t == 0) {
                tile_bones = (unsigned)bones;
                tile_discs = discs;
            }
        }
        __syncthreads();
    }

    const int y = y0t + t / (RENDER_TW / RENDER_PX);
    const int x = x0t + (t % (RENDER_TW / RENDER_PX)) * RENDER_PX;
    if (y >= H || x >= W) return;
    const int n = min(RENDER_PX, W - x);                 // pixels of this group inside the row
    const size_t pix = ((size_t)b * H + y) * W + x;      // of the group's first pixel, in out and in a uint8 canvas

    // ---- canvas
    float val[RENDER_PX][3];
    if (p.kind == DSNT_RENDER_CANVAS_F32) {
        const float* src = static_cast<const float*>(p.canvas);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* s = src + (((size_t)b * 3 + c) * H + y) * W + x;
            float raw[RENDER_PX] = {0.f, 0.f, 0.f, 0.f};
            if (n == RENDER_PX && ((uintptr_t)s & 15) == 0) {
                const float4 q = *reinterpret_cast<const float4*>(s);
                raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
            } else {
                for (int k = 0; k < n; ++k) raw[k] = s[k];
            }
#pragma unroll
            for (int k = 0; k < RENDER_PX; ++k) {
                const float un = raw[k] * p.stdv[c] + p.mean[c];                 // two roundings (no contraction)
                val[k][c] = fminf(fmaxf(un * 255.f, 0.f), 255.f);
            }
        }
    } else if (p.kind == DSNT_RENDER_CANVAS_U8) {
        const uint8_t* s = static_cast<const uint8_t*>(p.canvas) + pix * 3;
        uint32_t word[3] = {0u, 0u, 0u};
        if (n == RENDER_PX && ((uintptr_t)s & 3) == 0) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
            word[0] = s4[0]; word[1] = s4[1]; word[2] = s4[2];
        } else {
            for (int i = 0; i < 3 * n; ++i) word[i >> 2] |= (uint32_t)s[i] << (8 * (i & 3));
        }
#pragma unroll
        for (int k = 0; k < RENDER_PX; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * k + c;
                val[k][c] = (float)((word[i >> 2] >> (8 * (i & 3))) & 0xffu);
            }
    } else {
#pragma unroll
        for (int k = 0; k < RENDER_PX; ++k) val[k][0] = val[k][1] = val[k][2] = 0.f;
    }

    // ---- heat-map layer
    if (p.nheat > 0) {
        const int h = p.h, w = p.w;
        const bool native = h == H && w == W;
        // source rows and columns of the group: src = (dst + 0.5) * h / H - 0.5, clamped to the map
        const float sy = fminf(fmaxf(((float)y + 0.5f) * ((float)h / (float)H) - 0.5f, 0.f), (float)(h - 1));
        const int ya = native ? y : (int)sy, yb = min(ya + 1, h - 1);
        const float fy = native ? 0.f : sy - (float)ya;
        int xa[RENDER_PX], xb[RENDER_PX];
        float fx[RENDER_PX];
#pragma unroll
        for (int k = 0; k < RENDER_PX; ++k) {
            const int xk = min(x + k, W - 1);
            const float sx = fminf(fmaxf(((float)xk + 0.5f) * ((float)w / (float)W) - 0.5f, 0.f), (float)(w - 1));
            xa[k] = native ? xk : (int)sx;
            xb[k] = min(xa[k] + 1, w - 1);
            fx[k] = native ? 0.f : sx - (float)xa[k];
        }
        float heat[RENDER_PX][3];
#pragma unroll
        for (int k = 0; k < RENDER_PX; ++k) heat[k][0] = heat[k][1] = heat[k][2] = 0.f;
        for (int q = 0; q < p.nheat; ++q) {
            const int j = heat_j[q];
            const float pk = p.peak[((size_t)b * J + j) * p.peak_stride];
            const bool ok = pk > 0.f && isfinite(pk);
            const float* m = p.hm + ((size_t)b * J + j) * h * w;
            const float* ra = m + (size_t)ya * w;
            const float* rb = m + (size_t)yb * w;
            const float cr = heat_c[q][0], cg = heat_c[q][1], cb = heat_c[q][2];
#pragma unroll
            for (int k = 0; k < RENDER_PX; ++k) {
                float s;
                if (native) {
                    s = ra[xa[k]];
                } else {
                    const float top = ra[xa[k]] * (1.f - fx[k]) + ra[xb[k]] * fx[k];
                    const float bot = rb[xa[k]] * (1.f - fx[k]) + rb[xb[k]] * fx[k];
                    s = top * (1.f - fy) + bot * fy;
                }
                const float v = ok ? clamp01(s / pk) : 0.f;
                heat[k][0] += v * cr;
                heat[k][1] += v * cg;
                heat[k][2] += v * cb;
            }
        }
#pragma unroll
        for (int k = 0; k < RENDER_PX; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) val[k][c] = val[k][c] + (255.f - val[k][c]) * (p.heat_alpha * clamp01(heat[k][c]));
    }

    // ---- skeleton layer: the tile's bones in table order, then its discs in joint order
    if (p.nbones > 0) {
        const float cy = (float)y + 0.5f;
        unsigned bones = __builtin_amdgcn_readfirstlane(tile_bones);
        while (bones) {
            const int k = __ffs(bones) - 1;
            bones &= bones - 1;
            const int j1 = bone_j[k] & 0xff, j2 = bone_j[k] >> 8;
            const float px = ju[j1], py = jv[j1];
            const float ex = ju[j2] - px, ey = jv[j2] - py;
            const float ee = ex * ex + ey * ey;
            const float inv_ee = ee > 0.f ? 1.f / ee : 0.f;
            const bool grey = ((jstate[j1] | jstate[j2]) & 2) != 0;
            const float r = grey ? 100.f : bone_c[k][0], g = grey ? 100.f : bone_c[k][1],
                        bl = grey ? 100.f : bone_c[k][2];
#pragma unroll
            for (int i = 0; i < RENDER_PX; ++i) cover(val[i], (float)(x + i) + 0.5f, cy, px, py, ex, ey, inv_ee, p.reach, r, g, bl);
        }
        unsigned long long discs = tile_discs;
        discs = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(discs >> 32)) << 32) |
                __builtin_amdgcn_readfirstlane((unsigned)discs);
        while (discs) {
            const int j = __ffsll((long long)discs) - 1;
            discs &= discs - 1;
            const int st = jstate[j];
            const int k = (st >> 8) - 1;
            const bool grey = (st & 2) != 0;
            const float r = grey ? 100.f : bone_c[k][0], g = grey ? 100.f : bone_c[k][1],
                        bl = grey ? 100.f : bone_c[k][2];
#pragma unroll
            for (int i = 0; i < RENDER_PX; ++i)
                cover(val[i], (float)(x + i) + 0.5f, cy, ju[j], jv[j], 0.f, 0.f, 0.f, p.disc_reach, r, g, bl);
        }
    }

    // ---- clamp, truncate, pack: byte 3k + c of the group = channel c of pixel x + k
    uint32_t word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < RENDER_PX; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int i = 3 * k + c;
            const uint32_t q = (uint32_t)(int)fminf(fmaxf(val[k][c], 0.f), 255.f);
            word[i >> 2] |= q << (8 * (i & 3));
        }
    uint8_t* o = p.out + pix * 3;
    if (n == RENDER_PX && ((uintptr_t)o & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = word[0];
        o4[1] = word[1];
        o4[2] = word[2];
    } else {                                 // a row that does not start on a dword (W % 4 != 0), or its last, partial group
        for (int i = 0; i < 3 * n; ++i) o[i] = (uint8_t)(word[i >> 2] >> (8 * (i & 3)));
    }
}

}  // namespace

extern "C" int dsnt_render_pose(const void* canvas, int canvas_kind, const float* mean, const float* stdv, int B, int H,
                                int W, int J, const float* heatmaps, int h, int w, const float* peak, int64_t peak_stride,
                                const float* heat_rgb, float heat_alpha, const float* coords, const float* mask,
                                int pixel_coords, const int32_t* bone_joints, const float* bone_rgb, int nbones,
                                float width, float joint_radius, uint8_t* out, void* stream) {
    const bool heat = heatmaps != nullptr, skel = nbones != 0;
    DSNT_REQUIRE(out, DSNT_ERR_ARG, "dsnt_render_pose: null out");
    DSNT_REQUIRE(canvas_kind == DSNT_RENDER_CANVAS_BLACK || canvas_kind == DSNT_RENDER_CANVAS_F32 ||
                 canvas_kind == DSNT_RENDER_CANVAS_U8, DSNT_ERR_SHAPE, "dsnt_render_pose: unknown canvas kind %d", canvas_kind);
    DSNT_REQUIRE(canvas_kind == DSNT_RENDER_CANVAS_BLACK || canvas, DSNT_ERR_ARG, "dsnt_render_pose: null canvas of kind %d",
                 canvas_kind);
    DSNT_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= DSNT_RENDER_MAX_SIDE && W <= DSNT_RENDER_MAX_SIDE,
                 DSNT_ERR_SHAPE, "dsnt_render_pose: bad shape B=%d H=%d W=%d", B, H, W);
    DSNT_REQUIRE(!heat || (peak && heat_rgb), DSNT_ERR_ARG, "dsnt_render_pose: a heat-map layer needs peak and heat_rgb (null)");
    DSNT_REQUIRE(!skel || (coords && bone_joints && bone_rgb), DSNT_ERR_ARG,
                 "dsnt_render_pose: a skeleton layer needs coords and the bone table (null)");
    DSNT_REQUIRE(!(heat || skel) || (J >= 1 && J <= DSNT_RENDER_MAX_JOINTS), DSNT_ERR_SHAPE,
                 "dsnt_render_pose: J=%d outside 1..%d", J, DSNT_RENDER_MAX_JOINTS);
    DSNT_REQUIRE(!heat || (h >= 1 && w >= 1 && h <= DSNT_RENDER_MAX_SIDE && w <= DSNT_RENDER_MAX_SIDE && peak_stride >= 1),
                 DSNT_ERR_SHAPE, "dsnt_render_pose: bad heat-map shape h=%d w=%d peak_stride=%lld", h, w, (long long)peak_stride);
    DSNT_REQUIRE(nbones >= 0 && nbones <= DSNT_RENDER_MAX_BONES, DSNT_ERR_SHAPE, "dsnt_render_pose: %d bones, at most %d",
                 nbones, DSNT_RENDER_MAX_BONES);
    DSNT_REQUIRE(!skel || width > 0.f, DSNT_ERR_SHAPE, "dsnt_render_pose: width %g must be positive", (double)width);

    RenderParams p;
    memset(&p, 0, sizeof(p));
    p.canvas = canvas; p.out = out;
    p.kind = canvas_kind; p.H = H; p.W = W; p.J = J;
    p.tiles_x = (W + RENDER_TW - 1) / RENDER_TW;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = mean ? mean[c] : 0.f;
        p.stdv[c] = stdv ? stdv[c] : 1.f;
    }
    if (heat) {
        for (int j = 0; j < J; ++j) {
            const float* c = heat_rgb + 3 * j;
            if (c[0] == 0.f && c[1] == 0.f && c[2] == 0.f) continue;            // a black joint adds nothing
            p.heat_joint[p.nheat] = (unsigned char)j;
            for (int i = 0; i < 3; ++i) p.heat_rgb[p.nheat][i] = c[i];
            ++p.nheat;
        }
        p.hm = heatmaps; p.peak = peak; p.peak_stride = peak_stride; p.h = h; p.w = w; p.heat_alpha = heat_alpha;
    }
    if (skel) {
        for (int k = 0; k < nbones; ++k) {
            const int j1 = bone_joints[2 * k], j2 = bone_joints[2 * k + 1];
            DSNT_REQUIRE(j1 >= 0 && j1 < J && j2 >= 0 && j2 < J, DSNT_ERR_SHAPE,
                         "dsnt_render_pose: bone %d joins joints %d and %d, outside 0..%d", k, j1, j2, J - 1);
            p.bone_j1[k] = (unsigned char)j1;
            p.bone_j2[k] = (unsigned char)j2;
            for (int i = 0; i < 3; ++i) p.bone_rgb[k][i] = bone_rgb[3 * k + i];
        }
        p.nbones = nbones; p.coords = coords; p.mask = mask; p.pixel_coords = pixel_coords;
        p.reach = width * 0.5f + 0.5f;
        p.disc_reach = joint_radius > 0.f ? joint_radius + 0.5f : 0.f;
    }
    const int tiles_y = (H + RENDER_TH - 1) / RENDER_TH;
    DSNT_LAUNCH(render_pose_kernel, dim3(p.tiles_x * tiles_y, B), dim3(RENDER_NT), 0, (hipStream_t)stream, p);
    DSNT_CHECK_LAUNCH("dsnt_render_pose");
}
