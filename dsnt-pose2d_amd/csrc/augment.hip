// The MPII training-sample transform on the device (reference src/dsnt/data.py:118-226), one launch per batch.
//
// dsnt_augment_fwd: src uint8 [B][R][R][3] (the crops MpiiData.load_cropped_image(id, size=R, margin=R/4) returns) ->
// input f32 [B][3][S][S], composed in the reference's order:
//   1. hflip: Image.transpose(FLIP_LEFT_RIGHT), i.e. flipped[y][x] = src[y][R-1-x].
//   2. rot != 0: Image.rotate(rot, BILINEAR), expand=False.  Pillow takes rot % 360 (Python's modulo), builds the
//      inverse map [a b c; d e f] from cos/sin of -radians(rot % 360) rounded to 15 decimals, centred on (R/2, R/2)
//      (c = a*(-R/2) + b*(-R/2) + R/2, f likewise), and for output pixel (x, y) samples xin = a*(x+.5) + b*(y+.5) + c,
//      yin = d*(x+.5) + e*(y+.5) + f in fp64.  Outside [0, R) x [0, R): black.  Inside: taps at floor(xin - .5),
//      floor(yin - .5) and +1, clamped to the image, lerped in fp64 along x then y (a + (b - a) * t), and the value
//      TRUNCATED to uint8 (the rotated image is a PIL uint8 image).  Verified bit-exact against Pillow 12.2.
//   3. torchvision 0.2.0 CenterCrop(R * scale): the size is int()-truncated, c = int(R * scale); center_crop takes
//      i = j = int(round((R - c) / 2.)) (Python 3 round: half to even) and Image.crop((j, i, j + c, i + c)), which
//      zero-fills where the box leaves the image (scale > 1).  So crop pixel (u, v) is rotated pixel (u + off, v + off).
//   4. ToTensor (q / 255 in fp32), x * gain[ch] (fp32), clamp(0, 1).
//   5. adaptive_avg_pool2d c x c -> S x S: window [floor(i*c/S), ceil((i+1)*c/S)), summed row-major in fp32, then
//      / kh / kw (ATen's CPU order).
//   6. Normalize: (x - mean[ch]) / std[ch] in fp32.
// One thread per output pixel: it walks its pool window in crop coordinates and maps each crop pixel back through the
// offset, the inverse rotation and the flip to one (bilinear) sample of src, which is read directly (a 442 KB source is
// L2-resident).  The three channel planes are written as coalesced stores.  No atomics, no inter-workgroup traffic:
// the output is bit-reproducible.  Built with -ffp-contract=off (build.py) so the fp64 sampling and the fp32 pooling
// round like Pillow's and ATen's separately rounded operations.
//
// draw != 0: the parameters are drawn on the device first, Philox4x32-10 keyed by (seed) with counter (sample, step, k),
// so no generator state is carried between calls, and written to scale/rot/hflip/gain (workgroup 0 of each sample
// writes; every workgroup computes the same draw).  Distributions (data.py:134-140): scale = 2^clip(N(0, .25), -.5, .5);
// rot = clip(N(0, 30), -60, 60) with probability 0.4, else 0; hflip ~ Bernoulli(.5); gain[ch] ~ U(.6, 1.4).
//
// dsnt_augment_keypoints (data.py:150-196, fp64): part_coords = t . matrix . [x, y, 1] with t = R(rot)/scale . F(hflip),
// joints permuted by the flip table under hflip (out[flip[j]] = in[j], as scatter_ does), part_mask permuted the same way
// and, in train mode, multiplied by |coord| < 1; trans_m / trans_b = the 2x2 / translation part of inv(matrix) . inv(t).
//
// Gather variants (dsnt_augment_fwd_gather, dsnt_augment_fwd_pair_gather, dsnt_augment_keypoints_gather): the same
// kernels instantiated with a Gather / KpGather argument.  Sample b reads row idx[b] of a resident pool of N samples
// instead of row b of a contiguous batch, and draws with sample word b + draw_offset (offset 0: exactly
// dsnt_augment_fwd's draw).  An index outside [0, N) reads nothing: that sample's input is NaN, its part_mask 0 and its
// coordinates, matrices and normalize NaN, so the loss (or NanGuard) reports it.  The instantiations without the
// argument are the kernels above, unchanged.
//
// dsnt_epoch_indices: out[i] = order(first + i), a bijection of [0, n) keyed by (seed, epoch); shuffle == 0 or n == 1:
// the identity.  Construction (restated in numpy by tests/loader_ref.py):
//   k = the smallest even number >= 2 with 2^k >= n; h = k / 2; mask = 2^h - 1.
//   feistel(x): L = x >> h, Rt = x & mask; for r in 0..7: (L, Rt) = (Rt, L ^ (F_r(Rt) & mask)); return (L << h) | Rt,
//     F_r(v) = word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter (v, epoch lo, epoch hi, 0x4F524400 + r).
//     The counter's last word is the domain: the augmentation draw uses 0, 1, 2 there, so order and draw are
//     independent streams of the same seed.
//   order(p) = y, where y = feistel(p), then y = feistel(y) while y >= n (cycle-walking: the walk stays on p's cycle
//     of the permutation of [0, 2^k), so it ends in [0, n); 2^k < 4n, about 4 steps or fewer expected).
//
// dsnt_crop_affine: R x R crops of full images, bit for bit Pillow's
//   Image.fromarray(img).transform((R, R), Image.AFFINE, (a, b, c, d, e, f), Image.BILINEAR)
// with the coefficients of the bounding-box matrix M (image pixels -> normalised crop coordinates in [-1, 1]^2; crop pixel
// centres at n = 2(x + .5)/R - 1).  inv = inverse3(M), the keypoints kernel's inverse, then in fp64 and in this order:
//   a = 2*inv[0]/R, b = 2*inv[1]/R, c = inv[2] - inv[0] - inv[1];  d = 2*inv[3]/R, e = 2*inv[4]/R, f = inv[5] - inv[3] - inv[4].
// Pillow samples crop pixel (x, y) at xin = a*(x+.5) + b*(y+.5) + c, yin = d*(x+.5) + e*(y+.5) + f with the bilinear rule
// of step 2 above (DSNT_BILINEAR_RGB), black outside the image.  Images come from a ragged pool (one uint8 HWC buffer,
// byte offset and (h, w) per image).  A sample whose index lies outside [0, N), whose image record does not fit the pool
// (a side outside [1, 16384], or bytes outside it) or whose det(M) is 0 or not finite reads nothing: its crop is zero and
// its valid byte 0.  Stores: a thread packs 4 pixels (12 bytes) into three dword stores, so a wave writes 768
// contiguous bytes; odd R (a crop not dword-aligned) and a crop's last partial group store bytes.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {

constexpr int AUG_NT = 256;

// (0, 1]: 24 random bits
__device__ inline double unit(uint32_t x) { return (double)((x >> 8) + 1u) * (1.0 / 16777216.0); }
__device__ inline double normal(uint32_t a, uint32_t b) {      // Box-Muller
    return sqrt(-2.0 * log(unit(a))) * cos(6.283185307179586 * unit(b));
}
__device__ inline double clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

__device__ void draw_params(uint64_t seed, uint64_t step, uint32_t b, float& scale, float& rot, uint8_t& hflip, float gain[3]) {
    uint32_t r0[4], r1[4], r2[4];
    Philox::gen(r0, seed, step, b, 0);
    Philox::gen(r1, seed, step, b, 1);
    Philox::gen(r2, seed, step, b, 2);
    scale = (float)exp2(clip(0.25 * normal(r0[0], r0[1]), -0.5, 0.5));
    rot = unit(r0[2]) <= 0.4 ? (float)clip(30.0 * normal(r1[0], r1[1]), -60.0, 60.0) : 0.f;
    hflip = unit(r0[3]) <= 0.5 ? 1 : 0;
    for (int ch = 0; ch < 3; ++ch) gain[ch] = (float)(0.6 + 0.8 * unit(r2[ch]));
}

// Pillow's rounding of the rotation coefficients: round(x, 15)
__device__ inline double round15(double x) { return rint(x * 1e15) / 1e15; }

// inv = inverse of the row-major 3 x 3 matrix m by the adjugate over the determinant; returns the determinant.  The one
// inverse of a bounding-box matrix: the keypoints kernel's back-projection and the crop kernel's sampling map both use it.
__device__ __forceinline__ double inverse3(const double* m, double inv[9]) {
    const double a00 = m[4] * m[8] - m[5] * m[7], a01 = m[2] * m[7] - m[1] * m[8], a02 = m[1] * m[5] - m[2] * m[4];
    const double a10 = m[5] * m[6] - m[3] * m[8], a11 = m[0] * m[8] - m[2] * m[6], a12 = m[2] * m[3] - m[0] * m[5];
    const double a20 = m[3] * m[7] - m[4] * m[6], a21 = m[1] * m[6] - m[0] * m[7], a22 = m[0] * m[4] - m[1] * m[3];
    const double det = m[0] * a00 + m[1] * a10 + m[2] * a20;
    inv[0] = a00 / det; inv[1] = a01 / det; inv[2] = a02 / det;
    inv[3] = a10 / det; inv[4] = a11 / det; inv[5] = a12 / det;
    inv[6] = a20 / det; inv[7] = a21 / det; inv[8] = a22 / det;
    return det;
}

// Pillow's bilinear sampler (bilinear_filter32RGB) at (XIN, YIN) of a W x H HWC uint8 image IMG: outside [0, W) x [0, H)
// it leaves q0..q2 as they are (the caller's black); inside, taps at floor(xin - .5), floor(yin - .5) and +1, clamped
// to the image (the second row only where it exists, else v2 = v1), lerped in fp64 along x then y (a + (b - a) * t) and
// truncated.  FLIP != 0: the taps of the image mirrored left-right.  A statement macro, not a function: as an inlined
// function the row address of augment_kernel compiled to different instructions, and augment_kernel keeps exactly the
// code it had before the crop kernel shared the sampler (hipcc -S).
#define DSNT_BILINEAR_RGB(IMG, W, H, XIN, YIN, FLIP, q0, q1, q2)                                  \
    do {                                                                                          \
        double xin = (XIN), yin = (YIN);                                                          \
        if (xin >= 0.0 && xin < (W) && yin >= 0.0 && yin < (H)) {                                  \
            xin -= 0.5;                                                                           \
            yin -= 0.5;                                                                           \
            const double fx = floor(xin), fy = floor(yin);                                        \
            const double dx = xin - fx, dy = yin - fy;                                            \
            const int xi = (int)fx, yi = (int)fy;                                                 \
            int xa = min(max(xi, 0), (W) - 1), xb = min(max(xi + 1, 0), (W) - 1);                 \
            if (FLIP) { xa = (W) - 1 - xa; xb = (W) - 1 - xb; }     /* taps of the flipped image */ \
            const int ya = min(max(yi, 0), (H) - 1);                                              \
            const bool has2 = yi + 1 >= 0 && yi + 1 < (H);          /* Pillow: else v2 = v1 */    \
            const uint8_t* ra = (IMG) + (size_t)ya * (W) * 3;                                     \
            const uint8_t* rb = has2 ? (IMG) + (size_t)(yi + 1) * (W) * 3 : ra;                   \
            int q[3];                                                                             \
            for (int ch = 0; ch < 3; ++ch) {                                                      \
                const double a0 = ra[xa * 3 + ch], a1 = ra[xb * 3 + ch];                          \
                const double v1 = a0 + (a1 - a0) * dx;                                            \
                const double b0 = rb[xa * 3 + ch], b1 = rb[xb * 3 + ch];                          \
                const double v2 = has2 ? b0 + (b1 - b0) * dx : v1;                                \
                q[ch] = (int)(v1 + (v2 - v1) * dy);                                               \
            }                                                                                     \
            q0 = q[0]; q1 = q[1]; q2 = q[2];                                                      \
        }                                                                                         \
    } while (0)

struct SampleCoef {
    double a, b, c, d, e, f;   // inverse rotation (Pillow's affine data)
    float gain[3], mean[3], std[3];
    int c_side, off, rotate, hflip;
};

// The gather variants' extra kernel argument: sample b is row idx[b] of a pool of n rows and draws with sample word
// b + draw_offset.  The kernels take it as an optional trailing parameter pack (`G... gather`, empty or one argument),
// so the instantiations without it have exactly the signature, and the code, of the plain kernels.
struct Gather {
    const int64_t* idx;
    int64_t n;
    uint32_t draw_offset;
};
struct KpGather {
    const int64_t* idx;
    int64_t n;
    const double* head_len;     // [n]
    double* normalize;          // [B]: head_len[idx[b]]
};
template <typename T>
__device__ inline const T& only(const T& t) { return t; }

// PAIR (dsnt_augment_fwd_pair): `out` is [2B][3][S][S] and every finished pixel is also stored at column S-1-x of sample
// B + b: the second half is exactly the first one mirrored (inference.py's reverse_tensor(input, -1)).
template <bool PAIR, typename... G>
__global__ void __launch_bounds__(AUG_NT) augment_kernel(const uint8_t* __restrict__ src, int R, int S,
                                                         float* __restrict__ scale_p, float* __restrict__ rot_p,
                                                         uint8_t* __restrict__ hflip_p, float* __restrict__ gain_p,
                                                         int draw, uint64_t seed, uint64_t step,
                                                         const float* __restrict__ mean, const float* __restrict__ stdv,
                                                         float* __restrict__ out, G... gather) {
    constexpr bool GATHER = sizeof...(G) > 0;
    __shared__ SampleCoef sc;
    const int b = blockIdx.y;
    uint32_t sample = (uint32_t)b;                    // the draw's sample word
    int64_t row = 0;                                  // (gather) the pool row of sample b; -1: outside the pool
    if constexpr (GATHER) {
        const Gather g = only(gather...);
        sample += g.draw_offset;
        row = g.idx[b];
        if (row < 0 || row >= g.n) row = -1;          // reads nothing; the sample's input becomes NaN below
    }
    if (threadIdx.x == 0) {
        float scale, rot, gain[3];
        uint8_t hflip;
        if (draw) {
            draw_params(seed, step, sample, scale, rot, hflip, gain);
            if (blockIdx.x == 0) {
                scale_p[b] = scale; rot_p[b] = rot; hflip_p[b] = hflip;
                for (int ch = 0; ch < 3; ++ch) gain_p[3 * b + ch] = gain[ch];
            }
        } else {
            scale = scale_p[b]; rot = rot_p[b]; hflip = hflip_p[b];
            for (int ch = 0; ch < 3; ++ch) gain[ch] = gain_p[3 * b + ch];
        }
        const double cd = (double)R * (double)scale;
        // scale is a device value the binding cannot check without a host sync, so the clamp is the contract: R * scale
        // below 1 or NaN gives a crop side of 1, above 8R a side of 8R (tests/test_augment_edges_gpu.py)
        const int c = cd >= 1.0 && cd <= 8.0 * R ? (int)cd : (cd > 1.0 ? 8 * R : 1);
        sc.c_side = c;
        sc.off = (int)rint((double)(R - c) / 2.0);
        sc.hflip = hflip != 0;
        double deg = fmod((double)rot, 360.0);
        if (deg < 0) deg += 360.0;                    // Python's float modulo
        sc.rotate = deg != 0.0;
        const double ang = -(deg * (M_PI / 180.0));
        const double ca = round15(cos(ang)), sa = round15(sin(ang));
        const double cx = R / 2.0, cy = R / 2.0;
        sc.a = ca; sc.b = sa; sc.d = -sa; sc.e = ca;
        sc.c = ca * -cx + sa * -cy + 0.0 + cx;
        sc.f = -sa * -cx + ca * -cy + 0.0 + cy;
        for (int ch = 0; ch < 3; ++ch) {
            sc.gain[ch] = gain[ch];
            sc.mean[ch] = mean[ch];
            sc.std[ch] = stdv[ch];
        }
    }
    __syncthreads();
    const int p = blockIdx.x * AUG_NT + threadIdx.x;
    if (p >= S * S) return;
    const int oy = p / S, ox = p - oy * S;
    if constexpr (GATHER) {
        if (row < 0) {
            const float nan = __builtin_nanf("");
            for (int half = 0; half < (PAIR ? 2 : 1); ++half) {
                float* o = out + ((size_t)half * gridDim.y + b) * 3 * S * S + p;
                o[0] = nan;
                o[(size_t)S * S] = nan;
                o[(size_t)2 * S * S] = nan;
            }
            return;
        }
    }
    const int c = sc.c_side, off = sc.off, flip = sc.hflip, rotate = sc.rotate;
    const int y0 = (int)(((long)oy * c) / S), y1 = (int)(((long)(oy + 1) * c + S - 1) / S);
    const int x0 = (int)(((long)ox * c) / S), x1 = (int)(((long)(ox + 1) * c + S - 1) / S);
    const uint8_t* img = GATHER ? src + (size_t)row * R * R * 3 : src + (size_t)b * R * R * 3;
    const float g0 = sc.gain[0], g1 = sc.gain[1], g2 = sc.gain[2];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int v = y0; v < y1; ++v) {
        const int Y = v + off;
        for (int u = x0; u < x1; ++u) {
            const int X = u + off;
            int q0 = 0, q1 = 0, q2 = 0;
            if (X >= 0 && X < R && Y >= 0 && Y < R) {
                if (!rotate) {
                    const uint8_t* px = img + ((size_t)Y * R + (flip ? R - 1 - X : X)) * 3;
                    q0 = px[0]; q1 = px[1]; q2 = px[2];
                } else {
                    const double xo = X + 0.5, yo = Y + 0.5;
                    DSNT_BILINEAR_RGB(img, R, R, sc.a * xo + sc.b * yo + sc.c, sc.d * xo + sc.e * yo + sc.f, flip, q0,
                                      q1, q2);
                }
            }
            s0 += fminf(fmaxf(((float)q0 / 255.f) * g0, 0.f), 1.f);
            s1 += fminf(fmaxf(((float)q1 / 255.f) * g1, 0.f), 1.f);
            s2 += fminf(fmaxf(((float)q2 / 255.f) * g2, 0.f), 1.f);
        }
    }
    const float kh = (float)(y1 - y0), kw = (float)(x1 - x0);
    float* o = out + (size_t)b * 3 * S * S + p;
    o[0] = (s0 / kh / kw - sc.mean[0]) / sc.std[0];
    o[(size_t)S * S] = (s1 / kh / kw - sc.mean[1]) / sc.std[1];
    o[(size_t)2 * S * S] = (s2 / kh / kw - sc.mean[2]) / sc.std[2];
    if (PAIR) {
        float* om = out + ((size_t)gridDim.y + b) * 3 * S * S + (size_t)oy * S + (S - 1 - ox);
        om[0] = o[0];
        om[(size_t)S * S] = o[(size_t)S * S];
        om[(size_t)2 * S * S] = o[(size_t)2 * S * S];
    }
}

// G: empty, or one KpGather (dsnt_augment_keypoints_gather: the inputs are rows idx[b] of the pools).
template <typename... G>
__global__ void augment_keypoints_kernel(const double* __restrict__ matrix, const double* __restrict__ kp,
                                         const float* __restrict__ kmask, const float* __restrict__ scale_p,
                                         const float* __restrict__ rot_p, const uint8_t* __restrict__ hflip_p,
                                         const int64_t* __restrict__ flip_idx, int train, int B, int J,
                                         float* __restrict__ part_coords, float* __restrict__ part_mask,
                                         double* __restrict__ trans_m, double* __restrict__ trans_b, G... gather) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * J) return;
    const int b = i / J, j = i - b * J;
    constexpr bool GATHER = sizeof...(G) > 0;
    const double* m = matrix + 9 * b;
    int64_t e = 0;                                    // (gather) the element of the pools: row idx[b], joint j
    if constexpr (GATHER) {
        const KpGather g = only(gather...);
        const int64_t row = g.idx[b];
        if (row < 0 || row >= g.n) {                  // reads nothing
            const double nan = __builtin_nan("");
            part_coords[2 * i] = part_coords[2 * i + 1] = (float)nan;
            part_mask[i] = 0.f;
            if (j == 0) {
                for (int e = 0; e < 4; ++e) trans_m[4 * b + e] = nan;
                trans_b[2 * b] = trans_b[2 * b + 1] = nan;
                g.normalize[b] = nan;
            }
            return;
        }
        if (j == 0) g.normalize[b] = g.head_len[row];
        m = matrix + 9 * row;
        e = row * J + j;
    }
    const double s = scale_p[b], rad = (double)rot_p[b] * (M_PI / 180.0);
    const double cs = cos(rad), sn = sin(rad);
    const bool flip = hflip_p[b] != 0;
    // t = [[cos/s, sin/s, 0], [-sin/s, cos/s, 0], [0, 0, 1]] . diag(flip ? -1 : 1, 1, 1)
    const double fx = flip ? -1.0 : 1.0;
    const double t00 = cs / s * fx, t01 = sn / s, t10 = -sn / s * fx, t11 = cs / s;
    const double x = GATHER ? kp[2 * e] : kp[2 * i], y = GATHER ? kp[2 * e + 1] : kp[2 * i + 1];
    const double px = m[0] * x + m[1] * y + m[2], py = m[3] * x + m[4] * y + m[5];
    const double qx = t00 * px + t01 * py, qy = t10 * px + t11 * py;
    int jo = flip ? (int)flip_idx[j] : j;
    if (jo < 0 || jo >= J) jo = j;                   // (the binding passes a permutation of 0..J-1; never write outside the row)
    part_coords[2 * (b * J + jo)] = (float)qx;
    part_coords[2 * (b * J + jo) + 1] = (float)qy;
    float mk = GATHER ? kmask[e] : kmask[i];
    if (train && !(fabs(qx) < 1.0 && fabs(qy) < 1.0)) mk *= 0.f;
    part_mask[b * J + jo] = mk;
    if (j == 0) {
        double inv[9];
        inverse3(m, inv);
        // inv(t) = diag(fx, 1, 1) . s * R^T = [[fx s cos, -fx s sin, 0], [s sin, s cos, 0], [0, 0, 1]]
        const double u00 = fx * s * cs, u01 = -fx * s * sn, u10 = s * sn, u11 = s * cs;
        trans_m[4 * b + 0] = inv[0] * u00 + inv[1] * u10;
        trans_m[4 * b + 1] = inv[0] * u01 + inv[1] * u11;
        trans_m[4 * b + 2] = inv[3] * u00 + inv[4] * u10;
        trans_m[4 * b + 3] = inv[3] * u01 + inv[4] * u11;
        trans_b[2 * b + 0] = inv[2];
        trans_b[2 * b + 1] = inv[5];
    }
}

// ImageSpecs.convert (data.py:38-56) on a float image: adaptive_avg_pool2d to S x S (ATen's windows and summation order, as
// in augment_kernel) then (x - mean[ch]) / std[ch].  One thread per output element of [N][C][S][S].
__global__ void __launch_bounds__(AUG_NT) pool_normalize_kernel(const float* __restrict__ x, int N, int C, int H, int W, int S,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ stdv, float* __restrict__ out) {
    const long i = (long)blockIdx.x * AUG_NT + threadIdx.x;
    if (i >= (long)N * C * S * S) return;
    const int ox = (int)(i % S), oy = (int)((i / S) % S), ch = (int)((i / ((long)S * S)) % C);
    const long plane = i / ((long)S * S);
    const int y0 = (int)(((long)oy * H) / S), y1 = (int)(((long)(oy + 1) * H + S - 1) / S);
    const int x0 = (int)(((long)ox * W) / S), x1 = (int)(((long)(ox + 1) * W + S - 1) / S);
    const float* xp = x + plane * H * W;
    float s = 0.f;
    for (int v = y0; v < y1; ++v)
        for (int u = x0; u < x1; ++u) s += xp[(long)v * W + u];
    out[i] = (s / (float)(y1 - y0) / (float)(x1 - x0) - mean[ch]) / stdv[ch];
}

// dsnt_epoch_indices (construction in the header comment).  h = half the Feistel width in bits; h == 0: the identity.
constexpr int ORDER_NT = 256;
constexpr int ORDER_ROUNDS = 8;
constexpr uint32_t ORDER_DOMAIN = 0x4F524400u;   // Philox counter word 3; the augmentation draw uses 0, 1, 2

__device__ inline uint64_t feistel(uint64_t x, int h, uint64_t seed, uint64_t epoch) {
    const uint64_t mask = (1ULL << h) - 1;
    uint64_t l = x >> h, r = x & mask;
    for (int i = 0; i < ORDER_ROUNDS; ++i) {
        uint32_t o[4];
        Philox::gen(o, seed, epoch, (uint32_t)r, ORDER_DOMAIN + i);
        const uint64_t t = l ^ (o[0] & mask);
        l = r;
        r = t;
    }
    return (l << h) | r;
}

__global__ void __launch_bounds__(ORDER_NT) epoch_indices_kernel(int64_t n, uint64_t seed, uint64_t epoch, int64_t first,
                                                                 int64_t count, int h, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * ORDER_NT + threadIdx.x;
    if (i >= count) return;
    const uint64_t p = (uint64_t)(first + i);
    if (h == 0) {
        out[i] = (int64_t)p;
        return;
    }
    uint64_t y = feistel(p, h, seed, epoch);
    while (y >= (uint64_t)n) y = feistel(y, h, seed, epoch);      // cycle-walking: ends on p's cycle inside [0, n)
    out[i] = (int64_t)y;
}

// dsnt_crop_affine (contract in the header comment).  Workgroup (x, b) makes CROP_NT * CROP_PX pixels of crop b; thread 0
// derives the sample's Pillow coefficients once, every thread then samples CROP_PX consecutive pixels (row-major over the
// crop, so a group may wrap a row) and packs their 12 bytes into three dwords.
constexpr int CROP_NT = 256;
constexpr int CROP_PX = 4;                 // 4 RGB pixels = 12 bytes = 3 dwords per thread
constexpr int CROP_MAX_SIDE = 16384;

struct CropCoef {
    double a, b, c, d, e, f;               // Pillow's affine data: crop pixel centre -> image pixel
    int64_t off;                           // of the image in the pool (an offset, so the taps stay global loads)
    int w, h, ok;
};

__global__ void __launch_bounds__(CROP_NT) crop_affine_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes,
                                                              const int64_t* __restrict__ offset,
                                                              const int32_t* __restrict__ hw, int64_t N,
                                                              const int64_t* __restrict__ idx,
                                                              const double* __restrict__ matrix, int R,
                                                              uint8_t* __restrict__ out, uint8_t* __restrict__ valid) {
    __shared__ CropCoef sc;
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        int ok = 0;
        const int64_t i = idx[b];
        if (i >= 0 && i < N) {
            const int h = hw[2 * i], w = hw[2 * i + 1];
            const int64_t off = offset[i];
            if (h >= 1 && h <= CROP_MAX_SIDE && w >= 1 && w <= CROP_MAX_SIDE && off >= 0 &&
                off <= pool_bytes - (int64_t)h * w * 3) {
                double inv[9];
                const double det = inverse3(matrix + 9 * b, inv);
                if (det != 0.0 && isfinite(det)) {
                    const double r = (double)R;
                    sc.a = 2 * inv[0] / r; sc.b = 2 * inv[1] / r; sc.c = inv[2] - inv[0] - inv[1];
                    sc.d = 2 * inv[3] / r; sc.e = 2 * inv[4] / r; sc.f = inv[5] - inv[3] - inv[4];
                    sc.off = off;
                    sc.w = w;
                    sc.h = h;
                    ok = 1;
                }
            }
        }
        sc.ok = ok;
        if (blockIdx.x == 0) valid[b] = (uint8_t)ok;
    }
    __syncthreads();
    const int64_t npx = (int64_t)R * R;
    const int64_t p0 = ((int64_t)blockIdx.x * CROP_NT + threadIdx.x) * CROP_PX;
    if (p0 >= npx) return;
    uint32_t word[3] = {0u, 0u, 0u};       // byte 3k + ch of the group = channel ch of pixel p0 + k
    if (sc.ok) {
        const double ca = sc.a, cb = sc.b, cc = sc.c, cd = sc.d, ce = sc.e, cf = sc.f;
        const uint8_t* img = pool + sc.off;
        const int W = sc.w, H = sc.h;
#pragma unroll
        for (int k = 0; k < CROP_PX; ++k) {
            const int64_t p = p0 + k;
            if (p < npx) {
                const int y = (int)(p / R), x = (int)(p - (int64_t)y * R);
                const double xo = x + 0.5, yo = y + 0.5;
                int q0 = 0, q1 = 0, q2 = 0;
                DSNT_BILINEAR_RGB(img, W, H, ca * xo + cb * yo + cc, cd * xo + ce * yo + cf, 0, q0, q1, q2);
                const int q[3] = {q0, q1, q2};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int j = 3 * k + ch;
                    word[j >> 2] |= (uint32_t)q[ch] << (8 * (j & 3));
                }
            }
        }
    }
    uint8_t* o = out + ((size_t)b * npx + p0) * 3;
    if (p0 + CROP_PX <= npx && ((uintptr_t)o & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = word[0];
        o4[1] = word[1];
        o4[2] = word[2];
    } else {                               // odd R (unaligned crops) or the last, partial group of a crop
        for (int j = 0; j < 3 * CROP_PX && p0 + j / 3 < npx; ++j) o[j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
    }
}

}  // namespace

extern "C" int dsnt_augment_fwd(const uint8_t* src, int B, int R, int S, float* scale, float* rot_deg, uint8_t* hflip,
                                float* gain, int draw, uint64_t seed, uint64_t step, const float* mean, const float* stdv,
                                float* out, void* stream) {
    DSNT_REQUIRE(src && scale && rot_deg && hflip && gain && mean && stdv && out, DSNT_ERR_ARG,
                 "dsnt_augment_fwd: null pointer");
    DSNT_REQUIRE(B > 0 && B <= 65535 && R > 0 && R <= 8192 && S > 0 && S <= 4096, DSNT_ERR_SHAPE,
                 "dsnt_augment_fwd: bad shape B=%d R=%d S=%d", B, R, S);
    DSNT_LAUNCH(augment_kernel<false>, dim3((S * S + AUG_NT - 1) / AUG_NT, B), dim3(AUG_NT), 0, (hipStream_t)stream, src,
                R, S, scale, rot_deg, hflip, gain, draw, seed, step, mean, stdv, out);
    DSNT_CHECK_LAUNCH("dsnt_augment_fwd");
}

extern "C" int dsnt_augment_fwd_pair(const uint8_t* src, int B, int R, int S, float* scale, float* rot_deg,
                                     uint8_t* hflip, float* gain, int draw, uint64_t seed, uint64_t step,
                                     const float* mean, const float* stdv, float* out, void* stream) {
    DSNT_REQUIRE(src && scale && rot_deg && hflip && gain && mean && stdv && out, DSNT_ERR_ARG,
                 "dsnt_augment_fwd_pair: null pointer");
    DSNT_REQUIRE(B > 0 && B <= 65535 && R > 0 && R <= 8192 && S > 0 && S <= 4096, DSNT_ERR_SHAPE,
                 "dsnt_augment_fwd_pair: bad shape B=%d R=%d S=%d", B, R, S);
    DSNT_LAUNCH(augment_kernel<true>, dim3((S * S + AUG_NT - 1) / AUG_NT, B), dim3(AUG_NT), 0, (hipStream_t)stream, src,
                R, S, scale, rot_deg, hflip, gain, draw, seed, step, mean, stdv, out);
    DSNT_CHECK_LAUNCH("dsnt_augment_fwd_pair");
}

extern "C" int dsnt_augment_keypoints(const double* matrix, const double* keypoints, const float* keypoint_mask, int B,
                                      int J, const float* scale, const float* rot_deg, const uint8_t* hflip,
                                      const int64_t* flip_idx, int train, float* part_coords, float* part_mask,
                                      double* trans_m, double* trans_b, void* stream) {
    DSNT_REQUIRE(matrix && keypoints && keypoint_mask && scale && rot_deg && hflip && flip_idx && part_coords &&
                 part_mask && trans_m && trans_b, DSNT_ERR_ARG, "dsnt_augment_keypoints: null pointer");
    DSNT_REQUIRE(B > 0 && J > 0 && (long)B * J <= (1L << 30), DSNT_ERR_SHAPE, "dsnt_augment_keypoints: bad shape B=%d J=%d",
                 B, J);
    DSNT_LAUNCH(augment_keypoints_kernel<>, dim3((B * J + 255) / 256), dim3(256), 0, (hipStream_t)stream, matrix,
                keypoints, keypoint_mask, scale, rot_deg, hflip, flip_idx, train, B, J, part_coords, part_mask, trans_m,
                trans_b);
    DSNT_CHECK_LAUNCH("dsnt_augment_keypoints");
}

template <bool PAIR>
static int augment_fwd_gather(const char* name, const uint8_t* pool, int64_t N, const int64_t* idx, int B, int R, int S,
                              float* scale, float* rot_deg, uint8_t* hflip, float* gain, int draw, uint64_t seed,
                              uint64_t step, uint32_t draw_offset, const float* mean, const float* stdv, float* out,
                              void* stream) {
    DSNT_REQUIRE(pool && idx && scale && rot_deg && hflip && gain && mean && stdv && out, DSNT_ERR_ARG, "%s: null pointer",
                 name);
    DSNT_REQUIRE(N > 0 && B > 0 && B <= 65535 && R > 0 && R <= 8192 && S > 0 && S <= 4096, DSNT_ERR_SHAPE,
                 "%s: bad shape N=%lld B=%d R=%d S=%d", name, (long long)N, B, R, S);
    const Gather g{idx, N, draw_offset};
    DSNT_LAUNCH(augment_kernel<PAIR>, dim3((S * S + AUG_NT - 1) / AUG_NT, B), dim3(AUG_NT), 0, (hipStream_t)stream, pool,
                R, S, scale, rot_deg, hflip, gain, draw, seed, step, mean, stdv, out, g);
    DSNT_CHECK_LAUNCH(name);
}

extern "C" int dsnt_augment_fwd_gather(const uint8_t* pool, int64_t N, const int64_t* idx, int B, int R, int S,
                                       float* scale, float* rot_deg, uint8_t* hflip, float* gain, int draw,
                                       uint64_t seed, uint64_t step, uint32_t draw_offset, const float* mean,
                                       const float* stdv, float* out, void* stream) {
    return augment_fwd_gather<false>("dsnt_augment_fwd_gather", pool, N, idx, B, R, S, scale, rot_deg, hflip, gain, draw,
                                     seed, step, draw_offset, mean, stdv, out, stream);
}

extern "C" int dsnt_augment_fwd_pair_gather(const uint8_t* pool, int64_t N, const int64_t* idx, int B, int R, int S,
                                            float* scale, float* rot_deg, uint8_t* hflip, float* gain, int draw,
                                            uint64_t seed, uint64_t step, uint32_t draw_offset, const float* mean,
                                            const float* stdv, float* out, void* stream) {
    return augment_fwd_gather<true>("dsnt_augment_fwd_pair_gather", pool, N, idx, B, R, S, scale, rot_deg, hflip, gain,
                                    draw, seed, step, draw_offset, mean, stdv, out, stream);
}

extern "C" int dsnt_augment_keypoints_gather(const double* matrix_pool, const double* kp_pool, const float* mask_pool,
                                             const double* head_len_pool, int64_t N, const int64_t* idx, int B, int J,
                                             const float* scale, const float* rot_deg, const uint8_t* hflip,
                                             const int64_t* flip_idx, int train, float* part_coords, float* part_mask,
                                             double* trans_m, double* trans_b, double* normalize, void* stream) {
    DSNT_REQUIRE(matrix_pool && kp_pool && mask_pool && head_len_pool && idx && scale && rot_deg && hflip && flip_idx &&
                 part_coords && part_mask && trans_m && trans_b && normalize, DSNT_ERR_ARG,
                 "dsnt_augment_keypoints_gather: null pointer");
    DSNT_REQUIRE(N > 0 && B > 0 && J > 0 && (long)B * J <= (1L << 30) && N <= (1LL << 40) / J, DSNT_ERR_SHAPE,
                 "dsnt_augment_keypoints_gather: bad shape N=%lld B=%d J=%d", (long long)N, B, J);
    const KpGather g{idx, N, head_len_pool, normalize};
    DSNT_LAUNCH(augment_keypoints_kernel<KpGather>, dim3((B * J + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                matrix_pool, kp_pool, mask_pool, scale, rot_deg, hflip, flip_idx, train, B, J, part_coords, part_mask,
                trans_m, trans_b, g);
    DSNT_CHECK_LAUNCH("dsnt_augment_keypoints_gather");
}

extern "C" int dsnt_epoch_indices(int64_t n, uint64_t seed, uint64_t epoch, int64_t first, int64_t count, int shuffle,
                                  int64_t* out, void* stream) {
    DSNT_REQUIRE(out, DSNT_ERR_ARG, "dsnt_epoch_indices: null pointer");
    DSNT_REQUIRE(n > 0 && n <= (1LL << 62) && first >= 0 && count > 0 && count <= n - first &&
                 count <= (int64_t)INT32_MAX * ORDER_NT, DSNT_ERR_SHAPE,
                 "dsnt_epoch_indices: bad range n=%lld first=%lld count=%lld", (long long)n, (long long)first,
                 (long long)count);
    int k = 2;
    while ((1ULL << k) < (uint64_t)n) k += 2;
    DSNT_LAUNCH(epoch_indices_kernel, dim3((unsigned)((count + ORDER_NT - 1) / ORDER_NT)), dim3(ORDER_NT), 0,
                (hipStream_t)stream, n, seed, epoch, first, count, shuffle != 0 && n > 1 ? k / 2 : 0, out);
    DSNT_CHECK_LAUNCH("dsnt_epoch_indices");
}

extern "C" int dsnt_crop_affine(const uint8_t* pool, int64_t pool_bytes, const int64_t* offset, const int32_t* hw,
                                int64_t N, const int64_t* idx, const double* matrix, int B, int R, uint8_t* out,
                                uint8_t* valid, void* stream) {
    DSNT_REQUIRE(pool && offset && hw && idx && matrix && out && valid, DSNT_ERR_ARG, "dsnt_crop_affine: null pointer");
    DSNT_REQUIRE(pool_bytes > 0 && N > 0 && B > 0 && B <= 65535 && R > 0 && R <= 8192, DSNT_ERR_SHAPE,
                 "dsnt_crop_affine: bad shape pool_bytes=%lld N=%lld B=%d R=%d", (long long)pool_bytes, (long long)N, B,
                 R);
    constexpr int per_wg = CROP_NT * CROP_PX;
    DSNT_LAUNCH(crop_affine_kernel, dim3((R * R + per_wg - 1) / per_wg, B), dim3(CROP_NT), 0, (hipStream_t)stream, pool,
                pool_bytes, offset, hw, N, idx, matrix, R, out, valid);
    DSNT_CHECK_LAUNCH("dsnt_crop_affine");
}

extern "C" int dsnt_pool_normalize(const float* x, int N, int C, int H, int W, int S, const float* mean, const float* stdv,
                                   float* out, void* stream) {
    DSNT_REQUIRE(x && mean && stdv && out, DSNT_ERR_ARG, "dsnt_pool_normalize: null pointer");
    DSNT_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && S > 0 && S <= 4096 && (long)N * C * S * S <= (1L << 31) - AUG_NT &&
                 (long)N * C * H * W <= (1L << 40), DSNT_ERR_SHAPE, "dsnt_pool_normalize: bad shape");
    const long total = (long)N * C * S * S;
    DSNT_LAUNCH(pool_normalize_kernel, dim3((unsigned)((total + AUG_NT - 1) / AUG_NT)), dim3(AUG_NT), 0, (hipStream_t)stream,
                x, N, C, H, W, S, mean, stdv, out);
    DSNT_CHECK_LAUNCH("dsnt_pool_normalize");
}
