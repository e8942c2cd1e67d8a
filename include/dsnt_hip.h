/*
 * dsnt_hip.h — C ABI of libdsnt_hip.so: the MI355X (gfx950) device path of the
 * dsnt-pose2d hot path.
 *
 * The reference (anibali/dsnt-pose2d) has NO FFI layer: its device work is whatever
 * PyTorch 0.3.1 + cuDNN 7 execute underneath pure-Python modules.
 * Each entry point below therefore cites the reference *call site* whose device
 * work it replaces (paths relative to /root/reference/src/dsnt/).
 *
 * Conventions
 *  - plain pointers + sizes; every pointer is DEVICE memory owned by the caller
 *    (PyTorch's allocator); the library allocates nothing and the product entry points
 *    declared here keep no state except a thread-local error string;
 *  - all arithmetic is fp32; activations are NHWC ([N][H][W][C], C innermost);
 *    conv weights are OHWI ([Cout][R][S][Cin]); heat-maps for the DSNT head are
 *    planar rows ([rows = N*J][H*W]);
 *  - kernels are enqueued on `stream` (a hipStream_t passed as void*) and never
 *    synchronise, so calls can be captured into a hipGraph;
 *  - return value 0 = OK, otherwise a dsnt_status; dsnt_last_error() describes it.
 *    No C++ exception crosses this boundary.
 */
#ifndef DSNT_HIP_H
#define DSNT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DSNT_OK = 0,
    DSNT_ERR_SHAPE = 1,       /* unsupported / inconsistent shape */
    DSNT_ERR_ALIGN = 2,       /* pointer or channel count not 16-byte compatible */
    DSNT_ERR_ARG = 3,         /* null pointer / bad enum */
    DSNT_ERR_HIP = 4          /* hipGetLastError() after launch */
} dsnt_status;

/* What a launch leaves behind for the CONSUMERS of its output besides the output itself: fp16x3 operand bounds.
 * amax (may be NULL): a 64-float bound as dsnt_amax leaves it; the launch RAISES it to the max |value| it writes to its
 *         output (atomic max on the bit patterns of non-negative floats: the caller zeroes the 64 slots once per step) — the
 *         fp16x3 operand bound of a consumer that reads the output without a BatchNorm in between (skip projections, `lin`
 *         convolutions: hourglass.py:45-48,120-135), or of a data gradient written by a convolution epilogue.  With a
 *         bn_bwd_epilogue: max |dz| (what dsnt_bn_bwd_finalize_bound turns into the bound of a BatchNorm backward folded
 *         into dsnt_conv1x1_bwd_f16x3).
 * amax_bn (may be NULL): the same for max |relu?(value * amax_scale[c] + amax_shift[c])| — the operand a consumer with
 *         an EVAL-mode BatchNorm(+ReLU) prologue will form from this output (inference.py:38-48: the vectors come from
 *         running statistics, so they exist before the producer runs); amax_scale / amax_shift: [C], 16-byte aligned.
 * (Until round 3 this struct — then dsnt_out_bounds — also described a BatchNorm finalisation run by the launch's last
 * workgroup; slower than the separate dsnt_bn_finalize launches in every measurement of three rounds, removed in round 4.) */
typedef struct {
    float* amax;
    float* amax_bn; const float* amax_scale; const float* amax_shift; int amax_relu, reserved;
} dsnt_out_bounds;

/* BatchNorm finalisation folded into the prologue of the launch that CONSUMES the BatchNorm (the low-resolution
 * hourglass levels, /root/reference/src/dsnt/hourglass.py:33-43 between two 10-us convolutions: a separate
 * dsnt_bn_finalize launch costs the dependency chain ~8 us there, ~120 of them 1.0 ms of an hg2 step).  Every
 * workgroup sums partial[tiles][2][C] itself (fp64, fixed order), writes mean / invstd / scale / shift — which the
 * launch then reads as its in_scale / in_shift and backward reads later — and workgroup 0 moves the running
 * statistics.  Limits: C <= 256, tiles * C <= 16384 (dsnt_conv_fwd_pro_ok). */
typedef struct dsnt_bn_prologue {
    const float* partial; int tiles, C;
    int64_t M;                                   /* rows the sums run over */
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;     /* may be NULL */
    float momentum, eps;
    float* mean; float* invstd; float* scale; float* shift;
} dsnt_bn_prologue;

int dsnt_version(void);
const char* dsnt_last_error(void);

/* ------------------------------------------------------------------ DSNT head
 * rows = product of leading dims (N*J); each row is one H x W map, contiguous. */

/* model.py:24-45 `_hm_preact`: mode 0 softmax (F.softmax over H*W), 1 thresholded
 * softmax (nn.py:119-139; threshold, eps), 2 abs, 3 relu, 4 sigmoid (each / (sum+eps)). */
int dsnt_preact_fwd(const float* x, float* y, int64_t rows, int hw, int mode,
                    float threshold, float eps, void* stream);
/* backward of the same (nn.py:131-139 for the softmax forms: y*(g - sum(y*g))). */
int dsnt_preact_bwd(const float* x, const float* y, const float* gy, float* gx,
                    int64_t rows, int hw, int mode, float threshold, float eps, void* stream);

/* nn.py:25-78 `generate_xy` + `expectation_2d` + `dsnt`: coords[row] = (E[x], E[y]). */
int dsnt_expect_fwd(const float* hm, float* coords, int64_t rows, int h, int w, void* stream);
/* its backward: ghm[row][i] = gcoords.x * X_i + gcoords.y * Y_i. */
int dsnt_expect_bwd(const float* gcoords, float* ghm, int64_t rows, int h, int w, void* stream);

/* nn.py:168-205 `make_gauss`: out[row] = normalised Gaussian at coords[row], sigma. */
int dsnt_make_gauss(const float* coords, float* out, int64_t rows, int h, int w, float sigma,
                    void* stream);
/* its backward (autograd through nn.py:180-203; the reference's make_gauss is differentiable in `coords`):
 * g_coords[row] = sum_i g_out[row][i] * d out[row][i] / d coords[row]  (closed form, Gaussian re-evaluated). */
int dsnt_make_gauss_bwd(const float* coords, const float* g_out, float* g_coords, int64_t rows, int h, int w,
                        float sigma, void* stream);

/* 'fc' output strategy: out_fc = nn.Linear(H*W, 2) on the flattened heat-maps (model.py:222-223, 293-303, 196-198).
 * out[rows][2] = hm[rows][hw] . W[2][hw]^T + b[2];  backward: ghm (may be NULL), gW[2][hw], gb[2] (may be NULL),
 * overwritten, rows summed in order (deterministic). */
int dsnt_fc2_fwd(const float* hm, const float* w, const float* b, float* out, int64_t rows, int hw, void* stream);
int dsnt_fc2_bwd(const float* g, const float* hm, const float* w, float* ghm, float* gw, float* gb, int64_t rows,
                 int hw, void* stream);

/* nn.py:208-298 regularisers, per-row value before masked_average.
 * kind: 0 js, 1 kl, 2 mse, 3 var.  target = mu_t [rows][2]. */
int dsnt_reg_fwd(const float* hm, const float* target, float* per_row, int64_t rows, int h, int w,
                 float sigma, int kind, void* stream);
/* ghm[row] = g_row[row] * d(per_row)/d(hm). */
int dsnt_reg_bwd(const float* hm, const float* target, const float* g_row, float* ghm,
                 int64_t rows, int h, int w, float sigma, int kind, void* stream);
/* gmu[row][2] = g_row[row] * d(per_row)/d(target[row]) for kind 0..2: the reference's target Gaussian is
 * make_gauss(mu_t, ...) inside autograd (/root/reference/src/dsnt/nn.py:219-271), so its regularisers are differentiable
 * in the target means; the derivative through the target pixel is composed with make_gauss's backward in registers. */
int dsnt_reg_bwd_mu(const float* hm, const float* target, const float* g_row, float* gmu,
                    int64_t rows, int h, int w, float sigma, int kind, void* stream);

/* nn.py:97-116 `euclidean_loss` (per-point part): dist[i] = ||a_i - t_i||_2, d dims. */
int dsnt_euclid_fwd(const float* actual, const float* target, float* dist, int64_t n, int d,
                    void* stream);
/* ga = g_dist * (a - t) / dist  (un-guarded at dist == 0, like the reference). */
int dsnt_euclid_bwd(const float* actual, const float* target, const float* dist,
                    const float* g_dist, float* g_actual, int64_t n, int d, void* stream);

/* nn.py:81-94 `masked_average`: out[0] = sum(l*m)/clamp(sum m, 1); out[1] = that denominator.
 * mask may be NULL (plain mean with max(numel,1)). */
int dsnt_masked_avg_fwd(const float* losses, const float* mask, float* out2, int64_t n,
                        void* stream);
/* g_losses[i] = g_out[0] * m_i / denom  (denom read from out2[1]). */
int dsnt_masked_avg_bwd(const float* g_out, const float* mask, const float* out2,
                        float* g_losses, int64_t n, void* stream);

/* Fused head, forward: model.py:288-291 (softmax preact + dsnt) in one pass over the logits.
 * Writes normalised heat-maps and coords. */
int dsnt_head_fwd(const float* logits, float* hm, float* coords, int64_t rows, int h, int w,
                  void* stream);
/* Flip-merged head of test-time flip augmentation, batched: replaces the merge and head of inference.py:38-57
 * (cat/flip/index_select/add/divide, forward_part2, compute_coords and baddbmm per batch of ONE sample).
 * logits f32 [2B][J][h][w], the last stack's heat-map logits of a paired batch (rows B..2B-1: the mirrored inputs).
 * Per (b, j): m[y][x] = (L[b][j][y][x] + L[B+b][perm[j]][y][w-1-x]) / 2 (fp32), then
 *   strategy DSNT_FLIP_DSNT:  preact (0..4 = softmax, thresholded_softmax, abs, relu, sigmoid, with threshold and eps as
 *                             dsnt_preact_fwd takes them) and the DSNT expectation; the coordinates equal dsnt_head_fwd's
 *                             (softmax) or dsnt_preact_fwd + dsnt_expect_fwd's on the merged tensor, bit for bit;
 *   strategy DSNT_FLIP_GAUSS: the arg-max decode of dsnt_decode_heatmaps (use_neighbours = 1) of m (preact ignored).
 * Out: coords f32 [B][J][2] (normalised); img f64 [B][J][2] = transform_b[b] + coords . transform_m[b] computed in fp64
 * (transform_m f64 [B][2][2], transform_b f64 [B][1][2]); hm f32 [B][J][h][w] = the merged heat-maps (the normalised
 * ones for dsnt, m itself for gauss), or NULL.  perm: HOST int[J], a permutation of 0..J-1 (inference.HFLIP_INDICES),
 * J <= 32, passed by value to the kernel.  Maps as dsnt_head_fwd accepts.  dsnt_version() >= 116. */
#define DSNT_FLIP_DSNT 0
#define DSNT_FLIP_GAUSS 1
int dsnt_flip_merge_head(const float* logits, int64_t B, int J, int h, int w, const int* perm, int strategy,
                         int preact, float threshold, float eps, const double* transform_m, const double* transform_b,
                         float* hm, float* coords, double* img, void* stream);
/* Per-joint statistics of heat-maps (a confidence and a spread for every predicted joint).  hm f32 [rows][h][w], the
 * post-activation maps.  With the DSNT grid X = (2x + 1)/w - 1, Y = (2y + 1)/h - 1, per row:
 *   stats f32 [rows][7] = peak (max p), mass (sum p), mx = sum X p, my = sum Y p (dsnt_expect_fwd's values bit for bit),
 *                         vxx = sum (X - mx)^2 p, vyy = sum (Y - my)^2 p, vxy = sum (X - mx)(Y - my) p (a second sweep
 *                         about the mean, not raw moments);
 *   peak_index int32 [rows] = the first index y w + x that holds the peak (NaN is never the peak; 0 when nothing is
 *                         above -inf).
 * Forward only.  Maps as dsnt_expect_fwd accepts; rows of up to 4096 pixels are read once.  dsnt_version() >= 120. */
int dsnt_heatmap_stats(const float* hm, int64_t rows, int h, int w, float* stats, int* peak_index, void* stream);
/* dsnt_flip_merge_head with the statistics of the merged heat-maps from the same launch (no second read of the logits
 * for rows of up to 4096 pixels; longer rows read them twice).  coords, img and hm are dsnt_flip_merge_head's bit for bit.
 * stats [B J][7] and peak_index [B J] as dsnt_heatmap_stats gives them on hm (bit for bit, except mass, mean and cov of
 * softmax rows whose width is a multiple of 4, which are summed in the coordinates' order: fp32 rounding); cov_image f64 [B J][2][2] = M^T S M with
 * S = [[vxx, vxy], [vxy, vyy]] and M = transform_m[b]: the covariance of the joint in original-image pixels^2
 * (sqrt(trace) is its spread in pixels).  DSNT_FLIP_GAUSS: peak, peak_index and mass of the merged map as it is, the
 * rest NaN; peak and peak_index are the decode's own arg-max, so there a NaN in the map IS the peak (peak NaN,
 * peak_index its first NaN: dsnt_decode_heatmaps' rule, not dsnt_heatmap_stats').  All three outputs are required.
 * dsnt_version() >= 120. */
int dsnt_flip_merge_head_stats(const float* logits, int64_t B, int J, int h, int w, const int* perm, int strategy,
                               int preact, float threshold, float eps, const double* transform_m,
                               const double* transform_b, float* hm, float* coords, double* img, float* stats,
                               int* peak_index, double* cov_image, void* stream);
/* Fused head, loss: model.py:233-246 — per-row Euclidean distance and regulariser value
 * (reg_kind -1 = none) from the saved heat-maps; reductions by dsnt_masked_avg_fwd. */
int dsnt_head_loss_rows(const float* hm, const float* coords, const float* target,
                        float* dist, float* reg_row, int64_t rows, int h, int w, float sigma,
                        int reg_kind, void* stream);
/* Fused head, loss AND its gradient in one pass over the saved heat-maps (the train step; model.py:233-246,
 * train.py:358,381): per row the Euclidean distance and the regulariser value (as dsnt_head_loss_rows) and
 *   g_logits[row] = d( w_row (dist + reg_coeff reg) ) / d logits,  w_row = mask[row] / clamp(sum mask, 1)
 * (mask NULL: 1 / max(rows, 1) — nn.py:81-94), i.e. the gradient of this stack's loss for an upstream gradient of 1;
 * dsnt_scale_by_scalar applies another upstream value.  denom2 = the 2 floats dsnt_mask_denom left ({sum mask, its
 * clamp}: once per step, every stack shares the mask).  The head of a train step is then 4 HBM passes per stack
 * instead of 5.  H * W <= 4096. */
int dsnt_mask_denom(const float* mask, float* denom2, int64_t n, void* stream);
int dsnt_head_loss_grad(const float* hm, const float* coords, const float* target, const float* mask,
                        const float* denom2, float* dist, float* reg_row, float* g_logits, int64_t rows, int h, int w,
                        float sigma, int reg_kind, float reg_coeff, void* stream);
/* loss[0] = masked_average(dist) + reg_coeff * masked_average(reg_row) (reg_row NULL: no regulariser) in one launch;
 * e2 = {masked_average(dist), denominator} as dsnt_masked_avg_fwd leaves it. */
int dsnt_head_loss_reduce(const float* dist, const float* reg_row, const float* mask, const float* denom2,
                          float reg_coeff, float* loss, float* e2, int64_t rows, void* stream);
/* x[0..n) *= s[0] (device scalar); returns at once when s[0] == 1.  Any n > 0 and any alignment of x (16-byte stores
 * where x allows them); dsnt_version() >= 121, earlier versions refuse n % 4 != 0 and unaligned x. */
int dsnt_scale_by_scalar(float* x, const float* s, int64_t n, void* stream);
/* Fused head, backward: d loss / d logits in one pass, given per-row upstream factors
 * g_dist[row] (for the Euclidean term) and g_reg[row] (for the regulariser), i.e.
 * model.py:233-246 + nn.py:66-78 + softmax backward collapsed. */
int dsnt_head_bwd(const float* hm, const float* coords, const float* target, const float* dist,
                  const float* g_dist, const float* g_reg, float* g_logits, int64_t rows,
                  int h, int w, float sigma, int reg_kind, void* stream);
/* Heat-map distillation: per student row s and teacher row t of h x w LOGITS, temperature T > 0,
 *   lq = log_softmax(s / T), lp = log_softmax(t / T), q = exp(lq), p = exp(lp),
 *   kind 1 (kl):  loss_row = T^2 sum p (lp - lq)                      KL(teacher || student)
 *   kind 0 (js):  loss_row = T^2 (sum p (lp - lm) + sum q (lq - lm)) / 2,  lm = logaddexp(lp, lq) - ln 2
 *   kind 2 (mse): loss_row = T^2 sum (q - p)^2
 * formed in the log domain (no eps; a term whose p or q underflows contributes 0).  Student row r pairs with teacher
 * row r % teacher_rows (rows % teacher_rows == 0): a slab [S][B][J][h][w] reads a teacher [B][J][h][w] in place.
 * Any h * w < 2^24: rows of up to 4096 pixels are read from HBM once.  dsnt_version() >= 133. */
int dsnt_distill_rows(const float* student, const float* teacher, float* loss_row, int64_t rows, int64_t teacher_rows,
                      int h, int w, float temperature, int kind, void* stream);
/* The same loss_row AND the gradient with respect to the student's logits, the teacher a constant, in one launch, by
 * dsnt_head_loss_grad's convention (bit for bit the same loss_row when both calls take the same variant: always, unless
 * h * w % 4 == 0, student and teacher are 16-byte aligned and g_logits is not — this call then reads one float at a time):
 *   g_logits[row] = w_row d loss_row / d s,   w_row = mask[row] / denom2[1]   (mask NULL: 1 / rows, denom2 unused),
 *   d loss_row / d s_j = T (q_j - p_j) (kl),  T q_j (v_j - sum_i q_i v_i) with v = (lq - lm) / 2 (js), 2 (q - p) (mse);
 * a row of mask 0 gets a gradient of exactly 0.  denom2 = the 2 floats dsnt_mask_denom left; dsnt_scale_by_scalar
 * applies an upstream gradient other than 1.  dsnt_version() >= 133. */
int dsnt_distill_loss_grad(const float* student, const float* teacher, const float* mask, const float* denom2,
                           float* loss_row, float* g_logits, int64_t rows, int64_t teacher_rows, int h, int w,
                           float temperature, int kind, void* stream);

/* --------------------------------------------------------------- convolutions
 * Implicit-GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32).  Replaces nn.Conv2d forward
 * and its autograd (hourglass.py:20-25,104-105,120-123,135-136,148; model.py:129). */
typedef struct {
    int N, H, W, Cin;          /* input  [N][H][W][Cin]   (Cin % 4 == 0) */
    int Ho, Wo, Cout;          /* output [N][Ho][Wo][Cout] */
    int R, S;                  /* filter taps */
    int stride, pad, dil;
} dsnt_conv_geom;

/* y = conv(act(x)) + bias + res1 + res2,  act(x) = relu?(x*in_scale[c] + in_shift[c]) when
 * in_scale != NULL (the BatchNorm2d+ReLU that precedes the conv in a pre-activation
 * Bottleneck, hourglass.py:33-43, folded into the operand load; zero padding is applied
 * AFTER the activation, as F.conv2d pads the activated tensor).
 * bias/res1/res2 may be NULL.  res* have y's shape; res1 may alias y (in-place accumulate).
 * stats_partial (may be NULL): [ceil(M/128)][2][Cout] per-tile column sums and sums of
 * squares of y — the batch statistics of the next BatchNorm (hourglass.py:19,21,24). */
int dsnt_conv_fwd(const float* x, const float* w, const float* bias, float* y,
                  const float* in_scale, const float* in_shift, int in_relu,
                  const float* res1, const float* res2, float* stats_partial,
                  const dsnt_conv_geom* g, void* stream);

/* Data-gradient launches can fuse the first half of the BatchNorm+ReLU backward into the epilogue:
 * with `bnb` != NULL the kernel writes dz = (conv result) * [relu mask of bn(x)] to y and per-tile
 * (sum dz, sum dz*xhat) to stats_partial (xhat = (x - mean) * invstd), ready for
 * dsnt_bn_bwd_finalize; dsnt_bn_act_bwd_apply then runs with relu = 0 on dz. */
typedef struct {
    const float* x;            /* the BatchNorm input, shape of y */
    const float* scale; const float* shift; const float* mean; const float* invstd;   /* [C] */
    int relu;
} dsnt_bn_bwd_epilogue;
int dsnt_conv_fwd_ex(const float* x, const float* w, const float* bias, float* y,
                     const float* in_scale, const float* in_shift, int in_relu,
                     const float* res1, const float* res2, float* stats_partial,
                     const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail, void* stream);
/* (`tail`, here and in the other _ex variants: the operand bounds the launch leaves behind — dsnt_out_bounds.) */

/* dsnt_conv_fwd_ex with the BatchNorm of its A operand finalised in the launch's prologue (fp32-MFMA path: the
 * small-M kernels); in_scale / in_shift are pro->scale / pro->shift.  dsnt_conv_fwd_pro_ok(g, tiles, C) != 0 if the
 * limits hold for this geometry. */
int dsnt_conv_fwd_pro_ok(const dsnt_conv_geom* g, int tiles, int C);
int dsnt_conv_fwd_pro(const float* x, const float* w, const float* bias, float* y, const dsnt_bn_prologue* pro,
                      int in_relu, const float* res1, const float* res2, float* stats_partial,
                      const dsnt_conv_geom* g, const dsnt_out_bounds* tail, void* stream);

/* Rows per stats_partial tile that dsnt_conv_fwd uses for this geometry (128 or 32): the
 * caller sizes stats_partial as [ceil(M/bm)][2][Cout] and hands ceil(M/bm) to dsnt_bn_finalize. */
int dsnt_conv_fwd_bm(const dsnt_conv_geom* g);

/* bf16x6 variant: fp32-accurate convolution on the bf16 matrix cores.  Operands are split exactly
 * into three bf16 planes and the six product terms >= 2^-16 are accumulated in fp32 (error below
 * one fp32 rounding; 6/16 of the fp32-MFMA cost).  `w_planes` points at plane 0 of the OHWI weights
 * inside a dsnt_split_bf16x3 output; planes are `plane_stride` bf16 elements apart (a multiple of 8;
 * the whole parameter arena is split with one launch).  Every other argument as dsnt_conv_fwd.  Uses 128-row statistics
 * tiles.  dsnt_conv_bf16x6_ok(g) != 0 tells whether the geometry is supported. */
int dsnt_conv_bf16x6_ok(const dsnt_conv_geom* g);
int dsnt_split_bf16x3(const float* src, void* dst_planes, int64_t n, void* stream);
int dsnt_conv_fwd_bf16x6(const float* x, const void* w_planes, int64_t plane_stride, const float* bias, float* y,
                         const float* in_scale, const float* in_shift, int in_relu,
                         const float* res1, const float* res2, float* stats_partial,
                         const dsnt_conv_geom* g, void* stream);

int dsnt_conv_fwd_bf16x6_ex(const float* x, const void* w_planes, int64_t plane_stride, const float* bias,
                            float* y, const float* in_scale, const float* in_shift, int in_relu,
                            const float* res1, const float* res2, float* stats_partial,
                            const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail,
                            void* stream);

/* fp16x3 variant: x * s = h1 + h2 on TWO fp16 planes after a power-of-two scale, three MFMAs per product (error vs
 * fp64 below a plain fp32 GEMM's: conv_split.h; the split bit for bit: tests/split_ref.py).  a_bound / w_bound are DEVICE scalars >= the
 * largest |value| of the A operand AFTER its BN+ReLU prologue (or of x when there is none) and of the weights; the
 * kernels derive the scales from them (pow2: bound * scale in [2^13, 2^14)), so a loose bound is fine and a bound
 * that is too SMALL overflows fp16.  w_planes: two fp16 planes made by dsnt_split_f16x2 with the SAME w_bound.
 * Same arguments otherwise as dsnt_conv_fwd_bf16x6_ex.
 * A "device scalar" bound is DSNT_BOUND_SLOTS = 64 floats whose MAXIMUM is the bound (producers that find it with
 * atomics spread them over the slots; the others write the same value 64 times). */
int dsnt_conv_fwd_f16x3_ex(const float* x, const void* w_planes, int64_t plane_stride, const float* w_bound,
                           const float* a_bound, const float* bias, float* y, const float* in_scale,
                           const float* in_shift, int in_relu, const float* res1, const float* res2,
                           float* stats_partial, const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb,
                           const dsnt_out_bounds* tail, void* stream);
/* The same call for a 3x3 / stride 1 / pad 1 convolution whose weight planes are in the STREAM layout of
 * dsnt_f16_prep_weights (row flag): the symmetric persistent kernel of csrc/conv3s.hip (cuDNN's 3x3 forward / data gradient of
 * /root/reference/src/dsnt/hourglass.py:22-23).  Needs dsnt_conv_fwd_stream_ok(g) (H % 4 == 0 and W % 32 == 0, or H % 8 == 0 and
 * W % 16 == 0; Cin % 32 == 0 and <= 128, Cout 64 or 128, tensors < 2 GiB) and res2 == NULL; DSNT_ERR_SHAPE otherwise.  The
 * convolution sums are bit-identical to dsnt_conv_fwd_f16x3_ex's; stats_partial rows are one per 128-pixel patch (4 x 32, or 8 x 16 when W % 32 != 0): [N * H * W / 128][2][Cout].
 * in_relu (this entry point and dsnt_conv_fwd_f16x3_ex): bit 0 = ReLU in the prologue; bit 1 (DSNT_CONV_SHARE_CHIP): the launch runs on
 * a stream of its own beside other work — the persistent kernels (3x3 stream kernel, streaming 1x1 kernel) then start fewer
 * workgroups (3/2 per CU; half of the CUs), so that CUs with free LDS remain for the other streams.  Results unchanged. */
#define DSNT_CONV_SHARE_CHIP 2
int dsnt_conv_fwd_f16x3_stream(const float* x, const void* w_planes, int64_t plane_stride, const float* w_bound,
                               const float* a_bound, const float* bias, float* y, const float* in_scale,
                               const float* in_shift, int in_relu, const float* res1, const float* res2,
                               float* stats_partial, const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb,
                               const dsnt_out_bounds* tail, void* stream);
int dsnt_conv_fwd_stream_ok(const dsnt_conv_geom* g);
/* Introspection (tests' launch census): the form of the csrc/conv3s.hip kernel a stream launch of `mode` takes on geometry g with
 * this process's tuning — mode 0 / 1: forward or plain data gradient (without / with res1), 3: with bnb, 4:
 * dsnt_conv_dgrad_f16x3_stream_apply.  Bit 0: 128 output columns as two 64-column halves per patch (few patches), bit 1: the
 * v_mfma_f32_16x16x32_f16 form with the LDS-DMA weight ring, bit 2: 8 x 16 pixel patches (W % 32 != 0).  -1: not a stream
 * geometry.  (/root/reference/src/dsnt/hourglass.py:22-23,36-40 is what every form computes.)  dsnt_version() >= 113. */
int dsnt_conv_fwd_stream_form(const dsnt_conv_geom* g, int mode);
/* out[0..63] = bound slots whose maximum is max |src[i]|; dst = two fp16 planes (plane_stride elements apart) of src * pow2(bound). */
int dsnt_amax(const float* src, int64_t n, float* out, void* stream);
int dsnt_split_f16x2(const float* src, void* dst, int64_t n, int64_t plane_stride, const float* bound, void* stream);
/* The same for many tensors per launch (device tables of int64 rows):
 * dsnt_f16_prep_weights: row of `row_ints` values {src float*, dst fp16 plane-0*, bound float*, count (% 4 == 0), plane stride
 *   (elements), stream Cout, stream Cin} (row_ints == 5: the last two are absent and read as 0; dsnt_version() >= 110): bound = max|src|, dst = the two fp16 planes of src * pow2(bound) — every conv's weights once
 *   per step; stream Cout > 0: src is an OHWI 3x3 filter [Cout][3][3][Cin] (Cin % 16 == 0) and each plane is written in
 *   STREAM order [Cin / 16][9 taps][Cout][16] for dsnt_conv_fwd_f16x3_stream (0, 0: element order kept);
 * dsnt_f16_prep_bn_bounds: row {gamma float*, beta float*, out float*, C, bits of float sqrt(M)}:
 *   out = max_c(|gamma_c| sqrt(M) + |beta_c|), an upper bound of |relu?(bn(x))| for a TRAIN-mode BatchNorm over M samples. */
int dsnt_f16_prep_weights(const int64_t* table, int rows, int row_ints, void* stream);   /* row_ints: 7, or 5 (no stream columns) */
int dsnt_f16_prep_bn_bounds(const int64_t* table, int rows, void* stream);

/* Re-pack OHWI weights for the data-gradient pass: wd[Cin][R][S][Cout] with taps flipped,
 * so that dgrad(dy) == dsnt_conv_fwd(dy, wd) with pad' = dil*(R-1) - pad (stride 1). */
int dsnt_conv_pack_dgrad(const float* w, float* wd, int Cout, int R, int S, int Cin,
                         void* stream);

/* The same for every convolution of a backward pass in one launch.  table[nconv][6] (device, int32) =
 * {src offset into params, dst offset, Cout, R, S, Cin}; writes fp32 into out[dst..] and the exact
 * bf16x3 split into planes (plane stride = total elements). */
int dsnt_conv_pack_dgrad_all(const int* table, int nconv, const float* params, float* out,
                             void* planes, int64_t total, void* stream);

/* Weight / bias gradient: dw[Cout][R][S][Cin] = sum_m act(x)[m, (r,s,c)] * dy[m, cout],
 * dbias[cout] = sum_m dy.  `ws` is caller workspace of dsnt_conv_wgrad_ws_floats() floats (enough for ANY of the
 * weight-gradient entry points on that geometry; dsnt_conv_wgrad_f16x3_ws_floats is the exact size of that call).
 * accumulate: bit 0 adds into dw/dbias instead of overwriting; bit 1 (DSNT_WGRAD_SHARE_CHIP, split-precision kernels):
 * the launch shares the chip with a dependency chain on another stream (loss.backward() of bin/train.py:380: weight
 * gradients feed nothing downstream) and keeps to ONE workgroup per CU, so that the chain's small kernels find a slot
 * instead of waiting for the whole weight gradient to retire.
 * dw == NULL (and dbias == NULL): only the split-M partial slabs are written to `ws`; the caller keeps `ws`
 * alive and reduces later with dsnt_wgrad_reduce_all (one launch for many convolutions). */
#define DSNT_WGRAD_SHARE_CHIP 2
/* bit 2, with DSNT_WGRAD_SHARE_CHIP, 3x3 halo kernel: half as many slabs / workgroups again (128 four-wave workgroups) — for
 * launches in the middle of backward, where the stream they run on has slack and the dependency chain beside them does not */
#define DSNT_WGRAD_NARROW 4
int64_t dsnt_conv_wgrad_ws_floats(const dsnt_conv_geom* g);
int dsnt_conv_wgrad(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                    const float* dy, float* ws, float* dw, float* dbias, int accumulate,
                    const dsnt_conv_geom* g, void* stream);

/* bf16x6 variant of the weight gradient (same arguments and workspace; both operands are split into
 * bf16 planes while they are staged).  dsnt_conv_wgrad_bf16x6_ok(g) != 0 if supported. */
int dsnt_conv_wgrad_bf16x6_ok(const dsnt_conv_geom* g);
int dsnt_conv_wgrad_bf16x6(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                           const float* dy, float* ws, float* dw, float* dbias, int accumulate,
                           const dsnt_conv_geom* g, void* stream);

/* Deferred reduction of the slabs of `rows` convolutions in one launch.  table[rows][7] (device, int64) =
 * {ws pointer, dw pointer, dbias pointer or 0, splits, Cout*R*S*Cin, Cout, accumulate} with `splits` =
 * dsnt_conv_wgrad_splits(g); max_blocks >= ceil((Cout*K/4 + ceil(Cout/4)) / 64) of the largest row.
 * Same summation order as the reduction inside dsnt_conv_wgrad (bit-identical results). */
int dsnt_conv_wgrad_splits(const dsnt_conv_geom* g);
int dsnt_wgrad_reduce_all(const int64_t* table, int rows, int max_blocks, void* stream);

/* Grouped weight gradients: many (small) convolutions in ONE launch.  dsnt_conv_wgrad_desc writes an opaque
 * descriptor of dsnt_conv_wgrad_desc_bytes() bytes (host memory) for one bf16x6 weight gradient with a
 * BN(+ReLU) prologue (same arguments as dsnt_conv_wgrad_bf16x6 with dw == NULL: slabs only) and returns its
 * number of workgroups (> 0) or -error.  The caller copies the descriptors back to back into device memory
 * and calls dsnt_conv_wgrad_group(table, nconv, max_blocks >= the largest workgroup count); x, dy, scale/shift
 * and ws must stay untouched until then; reduce afterwards with dsnt_wgrad_reduce_all.  Bit-identical to the
 * per-convolution launches.  Replaces the per-layer autograd weight-gradient calls of
 * /root/reference/src/dsnt/bin/train.py:380 (loss.backward()) for the low-resolution hourglass levels. */
int dsnt_conv_wgrad_desc_bytes(void);
int dsnt_conv_wgrad_desc(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                         const float* dy, float* ws, const dsnt_conv_geom* g, void* desc_out);
int dsnt_conv_wgrad_group(const void* table, int nconv, int max_blocks, void* stream);

/* fp16x3 weight gradient (two fp16 planes per operand, three MFMAs per product, scales from the 64-slot bounds
 * a_bound >= max|act(x)| and g_bound >= max|dy|; the slabs are written already unscaled).  Same arguments otherwise as
 * dsnt_conv_wgrad_bf16x6; dsnt_conv_wgrad_desc_f16x3 is the descriptor form for dsnt_conv_wgrad_group (descriptors of
 * both kinds may share one table). */
int dsnt_conv_wgrad_f16x3(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                          const float* dy, float* ws, float* dw, float* dbias, int accumulate,
                          const float* a_bound, const float* g_bound, const dsnt_conv_geom* g, void* stream);
int dsnt_conv_wgrad_desc_f16x3(const float* x, const float* in_scale, const float* in_shift, int in_relu,
                               const float* dy, float* ws, const float* a_bound, const float* g_bound,
                               const dsnt_conv_geom* g, void* desc_out);
/* 3x3 / stride 1 / pad 1 convolutions with Cin % 64 == 0, Cout % 64 == 0 and W in {16, 32, 64, 128, ...}
 * (dsnt_conv_wgrad_halo_ok != 0: conv2 of every Bottleneck, /root/reference/src/dsnt/hourglass.py:22-23) run
 * dsnt_conv_wgrad_f16x3 as a HALO kernel: a workgroup owns 64 input channels x all nine taps x 128 output channels of a
 * strip of pixel rows, so each operand element is BatchNorm-transformed and split once instead of nine times.  It cuts
 * the pixels into its own slabs: size `ws` with dsnt_conv_wgrad_f16x3_ws_floats and reduce
 * dsnt_conv_wgrad_f16x3_splits slabs, both asked with the `accumulate` flags of the launch (a DSNT_WGRAD_SHARE_CHIP
 * launch runs as four-wave workgroups, one per CU, over half as many slabs; both fall back to the plain plan for every
 * other geometry). */
int dsnt_conv_wgrad_halo_ok(const dsnt_conv_geom* g);
/* Which kernel an fp16x3 launch of geometry g reaches (both bounds given, no second residual, no BatchNorm-backward epilogue).
 * wgrad = 0 (dsnt_conv_fwd_f16x3_ex): 1 streaming 1x1, 2 halo tile, 0 implicit GEMM; wgrad = 1 (dsnt_conv_wgrad_f16x3): 1 stem,
 * 2 halo, 3 1x1, 0 generic.  < 0: not supported. */
int dsnt_conv_f16x3_route(const dsnt_conv_geom* g, int wgrad);
int dsnt_conv_wgrad_f16x3_splits(const dsnt_conv_geom* g, int accumulate);
int64_t dsnt_conv_wgrad_f16x3_ws_floats(const dsnt_conv_geom* g, int accumulate);

/* Forward of a 1x1 / stride 1 convolution with >= 4096 rows on the second streaming kernel (csrc/fwd1.hip): the same contract as
 * dsnt_conv_fwd_f16x3_ex for these shapes (BN+ReLU prologue or a raw operand, bias, ONE residual, operand bounds, `tail`) except
 * for the statistics: stats_partial is [rows][2][Cout] with rows = dsnt_conv1x1_fwd_stats_rows(g, in_relu) — one row per
 * WORKGROUP (<= 512) instead of one per 128 pixels; hand `rows` to dsnt_bn_finalize as its ntiles.  The activations are
 * loaded as whole rows (16 bytes per lane) and staged through LDS once for all output columns, where the first streaming
 * kernel (gemm1.hip, behind dsnt_conv_fwd_f16x3_ex) loads a row per lane.  in_relu: bit 0 = ReLU, bit 1 = DSNT_CONV_SHARE_CHIP.
 * dsnt_conv1x1_fwd_ok(g) != 0: (Cin, Cout) in {(256, 128), (128, 256), (128, 128), (64, 64), (64, 128), (256, 256)},
 * N*H*W % 32 == 0 and >= 16384.  Replaces nn.Conv2d 1x1 forward + the BatchNorm2d + ReLU in front of it
 * (/root/reference/src/dsnt/hourglass.py:20,25,33-43,44-48,146-153). */
int dsnt_conv1x1_fwd_ok(const dsnt_conv_geom* g);
int dsnt_conv1x1_fwd_stats_rows(const dsnt_conv_geom* g, int in_relu);
int dsnt_conv1x1_fwd_f16x3(const float* x, const void* w_planes, int64_t plane_stride, const float* w_bound,
                           const float* a_bound, const float* bias, float* y, const float* in_scale,
                           const float* in_shift, int in_relu, const float* res1, float* stats_partial,
                           const dsnt_conv_geom* g, const dsnt_out_bounds* tail, void* stream);
/* conv3 of a Bottleneck WITH a projection shortcut, and that shortcut, in one launch of the same kernel
 * (the reference's hourglass.py:25,44-48: `out = self.conv3(out); residual = self.downsample(x); out += residual`):
 *   y = conv(relu?(x in_scale + in_shift)) + bias + (conv_ds(x_ds) + bias_ds)
 * — what dsnt_conv1x1_fwd_f16x3(x_ds, ..., skip) followed by dsnt_conv1x1_fwd_f16x3(x, ..., res1 = skip) leave in y, its
 * statistics rows and its `tail`, bit for bit (two accumulator sets, one per operand pair with its own bounds; the shortcut's
 * value rounded to fp32 before it is added), without the skip tensor: 537 MB instead of 1075 MB for 64 -> 128 channels at
 * 128 x 128, batch 32.  Both convolutions have the same geometry (g_ds == g in Cin, Cout and pixels: DSNT_ERR_SHAPE otherwise) and
 * their weight planes the same plane_stride; (Cin, Cout) in {(64, 128), (128, 256)}.  Called by dsnt/engine.py `_conv_forward_ds`. */
int dsnt_conv1x1_fwd_ds_f16x3(const float* x, const float* x_ds, const void* w_planes, const void* w_planes_ds,
                              int64_t plane_stride, const float* w_bound, const float* w_bound_ds, const float* a_bound,
                              const float* a_bound_ds, const float* bias, const float* bias_ds, float* y,
                              const float* in_scale, const float* in_shift, int in_relu, float* stats_partial,
                              const dsnt_conv_geom* g, const dsnt_conv_geom* g_ds, const dsnt_out_bounds* tail, void* stream);
/* The stem (hourglass.py:157 `self.conv1`, 7x7 / stride 2 / pad 3 on the image) in its space-to-depth form: a 4x4 / stride 1 /
 * pad 1 convolution of the 16-channel image dsnt_s2d_input leaves ([N][H/2+1][W/2+1][16]), 64 output channels, fp16x3 — on a halo
 * kernel of its own (csrc/stem4.hip: the 7 x 35 input halo of a 4 x 32 output patch staged once for all 16 taps, weights in
 * registers).  dsnt_stem4_fwd_ok(g): 4x4, stride 1, pad 1, Cin 16, Cout 64, Ho % 4 == 0, Wo % 32 == 0.  Statistics: ONE row per
 * workgroup — dsnt_stem4_fwd_stats_rows(g) rows of [2][64], handed to dsnt_bn_finalize as ntiles.  w_planes: the plain
 * [Cout][4][4][16] planes of dsnt_s2d_weights_prep / dsnt_split_f16x2; tail: dsnt_out_bounds.amax only. */
int dsnt_stem4_fwd_ok(const dsnt_conv_geom* g);
int dsnt_stem4_fwd_stats_rows(const dsnt_conv_geom* g);
int dsnt_stem4_fwd_f16x3(const float* x, const void* w_planes, int64_t plane_stride, const float* w_bound,
                         const float* a_bound, const float* bias, float* y, float* stats_partial,
                         const dsnt_conv_geom* g, const dsnt_out_bounds* tail, void* stream);


/* The WHOLE backward of a 1x1 / stride 1 convolution y = conv(relu?(bn(x))) in one pass over its tensors — what
 * autograd runs as cuDNN backward-data + backward-filter of /root/reference/src/dsnt/hourglass.py:20,25 (conv1 / conv3 of
 * every Bottleneck) plus, with `ap`, the BatchNorm backward of the layer behind (hourglass.py:21,36-37):
 *   dz_out[m][c]  = (sum_n dY[m][n] W[n][c]) * [bn(x) > 0]     (the ReLU mask as dsnt_bn_bwd_epilogue defines it: xs)
 *   stats_partial = [splits][2][Cin] partial (sum dz_out, sum dz_out * xhat) for dsnt_bn_bwd_finalize (ntiles = splits)
 *   ws            = [splits][Cout][Cin] slabs of dW[n][c] = sum_m dY[m][n] act(x)[m][c], then [splits][Cout] bias partials
 *                   (reduce with dsnt_wgrad_reduce_all, `splits` = dsnt_conv1x1_bwd_splits(g))
 * dY is `dy` itself (ap == NULL) or is formed in registers from dy = dz of the BatchNorm that consumes y:
 *   dY = ap->scale * (dz - coef[0] - (y - mean) * invstd * coef[1])          (dsnt_bn_act_bwd_apply's arithmetic; that
 * launch and its 12 bytes per element disappear).  xs->x is read ONCE (mask, xhat and weight-gradient operand from the
 * same registers), dy (and ap->y) once: 402 MB instead of 737 MB for 256 -> 128 channels at 64 x 64, batch 32.
 * wd_planes: the data-gradient weights [Cin][Cout] (dsnt_conv_pack_dgrad) as two fp16 planes with bound w_bound
 * (dsnt_f16_prep_weights); a_bound >= max|act(x)|, g_bound >= max|dY| (64-slot bounds; with `ap`:
 * dsnt_bn_bwd_finalize_bound leaves it); dz_amax (may be NULL): raised to max|dz_out|.  flags: DSNT_CONV_SHARE_CHIP = the launch
 * runs on a stream of its own beside other work and keeps to half of the CUs (`splits` / ws size are asked with the same flags).
 * A convolution WITHOUT a BatchNorm in front of it (the projection shortcuts hourglass.py:44-48, the `fc` convolutions :146-153):
 * xs->scale == NULL (then shift / mean / invstd NULL too, ap == NULL, stats_partial unused): act(x) = x, dz_out = dL/dx itself,
 * added to what dz_out holds when bit 0 of `flags` is set.
 * dsnt_conv1x1_bwd_ok(g) != 0: (Cout, Cin) in {(128, 256), (256, 128), (128, 128), (64, 64), (128, 64), (256, 256)},
 * N*H*W % 32 == 0 and >= 16384. */
typedef struct {
    const float* y;            /* the convolution's own output = the BatchNorm's input, [M][Cout] */
    const float* scale; const float* mean; const float* invstd;   /* [Cout] */
    const float* coef;         /* [2][Cout] as dsnt_bn_bwd_finalize leaves it */
} dsnt_bn_bwd_apply;
int dsnt_conv1x1_bwd_ok(const dsnt_conv_geom* g);
int dsnt_conv1x1_bwd_splits(const dsnt_conv_geom* g, int flags);
int64_t dsnt_conv1x1_bwd_ws_floats(const dsnt_conv_geom* g, int flags);
int dsnt_conv1x1_bwd_f16x3(const dsnt_bn_bwd_epilogue* xs, const float* dy, const dsnt_bn_bwd_apply* ap,
                           const void* wd_planes, int64_t plane_stride, const float* w_bound, const float* a_bound,
                           const float* g_bound, float* dz_out, float* stats_partial, float* ws, float* dz_amax,
                           int flags, const dsnt_conv_geom* g, void* stream);
/* Data gradient of a 3x3 / stride 1 / pad 1 convolution whose OUTPUT y feeds a train-mode BatchNorm (conv2 of a Bottleneck,
 * /root/reference/src/dsnt/hourglass.py:36-40: bn3 behind conv2), with that BatchNorm's backward folded into the operand load
 * (csrc/conv3s.hip MODE 4): replaces dsnt_bn_act_bwd_apply(dz, y, ...) -> dy followed by dsnt_conv_fwd_f16x3_stream(dy, ...).
 *   dz      [N,H,W,C]  dL/d relu(bn(y)), ReLU-masked, its two BatchNorm sums already reduced into ap->coef = [c0 | c1]
 *   ap      the BatchNorm behind the convolution: y, scale (= gamma invstd), mean, invstd, coef (struct below)
 *   dy_out  [N,H,W,C]  receives dL/dy = scale (dz - c0 - (y - mean) invstd c1) (every pixel once); must not alias dz
 *   a_bound a bound of |dL/dy| (dsnt_bn_bwd_finalize_bound); w_planes / plane_stride / w_bound: the data-gradient filter in
 *           STREAM layout, as for dsnt_conv_fwd_f16x3_stream
 *   dx_dz, stats_partial, bnb (required), tail: the launch's output — the gradient behind the BatchNorm IN FRONT of the
 *           convolution, masked and with its two sums per 128-pixel patch — exactly as dsnt_conv_fwd_f16x3_stream with bnb
 *   flags   DSNT_CONV_SHARE_CHIP or 0
 * Needs dsnt_conv_fwd_stream_ok(g); DSNT_ERR_SHAPE otherwise.  dsnt_version() >= 112. */
int dsnt_conv_dgrad_f16x3_stream_apply(const float* dz, const dsnt_bn_bwd_apply* ap, float* dy_out,
                                       const void* w_planes, int64_t plane_stride, const float* w_bound,
                                       const float* a_bound, float* dx_dz, float* stats_partial, int flags,
                                       const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb,
                                       const dsnt_out_bounds* tail, void* stream);

/* ----------------------------------------------------- heat-map matching ("gauss" output strategy)
 * Rows = (image, joint) maps of h x w floats, target = normalised coordinates [rows][2].
 * dsnt_encode_heatmaps: /root/reference/src/dsnt/util.py:129-147 (encode_heatmaps) + :70-126 (draw_gaussian with
 *   clip_size 7, unnormalised): pixel = round_half_even((c + 1) * size/2 - 0.5), bump exp(-d^2 / (2 sigma^2)) on
 *   the 7x7 window, nothing when the centre lies more than 3.5 px outside the map.
 * dsnt_heatmap_mse_fwd: per_row[r] = sum_hw (hm - encode(target))^2 without materialising the target; the caller
 *   sums the rows and divides by rows*h*w (nn.functional.mse_loss of model.py:156 / :256).
 * dsnt_heatmap_mse_bwd: dhm = gscale[0] * 2 / (rows*h*w) * (hm - encode(target)); gscale is a device scalar.
 * dsnt_decode_heatmaps: util.py:150-198 (get_preds + decode_heatmaps): first arg-max pixel ((0,0) when the
 *   maximum is not positive; y = index / h as the reference), optional quarter-pixel shift towards the larger
 *   neighbour, then (p + 0.5) * 2/size - 1.  coords [rows][2].  The arg-max is torch.max's: a NaN is the maximum
 *   (the first one's index the arg-max), so a row that holds a NaN decodes to pixel (0,0) as it does in the
 *   reference. */
int dsnt_encode_heatmaps(const float* target, float* out, int64_t rows, int h, int w, float sigma, void* stream);
int dsnt_heatmap_mse_fwd(const float* hm, const float* target, float* per_row, int64_t rows, int h, int w,
                         float sigma, void* stream);
int dsnt_heatmap_mse_bwd(const float* hm, const float* target, const float* gscale, float* dhm, int64_t rows,
                         int h, int w, float sigma, void* stream);
int dsnt_decode_heatmaps(const float* hm, float* coords, int64_t rows, int h, int w, int use_neighbours,
                         void* stream);

/* ----------------------------------------------------- batch-norm, elementwise
 * x viewed as [M][C] (M = N*H*W), C % 4 == 0. */

/* Column sums / sums of squares per 128-row tile: partial[ceil(M/128)][2][C]
 * (same format as dsnt_conv_fwd's stats_partial). */
int dsnt_bn_stats(const float* x, float* partial, int64_t M, int C, void* stream);

/* nn.BatchNorm2d forward bookkeeping (hourglass.py:19,21,24,106,147; torch defaults):
 * training: mean/var(biased) from partials -> mean, invstd = rsqrt(var+eps);
 *           running_mean/var updated with `momentum` (unbiased var);
 * eval:     mean/invstd from the running statistics.
 * Always: scale = gamma*invstd, shift = beta - mean*scale. */
int dsnt_bn_finalize(const float* partial, int ntiles, int64_t M, int C,
                     const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps,
                     int training, float* mean, float* invstd, float* scale, float* shift,
                     void* stream);

/* y = relu?(x*scale + shift) materialised (stem: hourglass.py:158-159). */
int dsnt_bn_act_fwd(const float* x, const float* scale, const float* shift, int relu,
                    float* y, int64_t M, int C, void* stream);

/* Eval-mode (running statistics) BatchNorm vectors of many layers in ONE launch: table rows of int64
 * {gamma*, beta*, running_mean*, running_var*, mean*, invstd*, scale*, shift*, C, bits of float eps}; per row what
 * dsnt_bn_finalize(training = 0) writes (inference.py:33-48 runs the model in eval mode). */
int dsnt_bn_eval_prep(const int64_t* table, int rows, void* stream);
/* Backward of y = relu?(bn(x)) given da = dL/dy, in three steps:
 *  reduce:   partial[tile][0][c] = sum dz, partial[tile][1][c] = sum dz*xhat,
 *            dz = da * (y > 0), xhat = (x - mean)*invstd;
 *  finalize: dgamma (+)= sum dz*xhat, dbeta (+)= sum dz, coef[0][c] = mean(dz),
 *            coef[1][c] = mean(dz*xhat);
 *  apply:    dx (+)= gamma*invstd * (dz - coef0 - xhat*coef1).
 * `accumulate` of dsnt_bn_bwd_finalize: bit 0 = add to dgamma / dbeta; DSNT_BN_FROZEN = the forward ran on FIXED statistics
 * (nn.BatchNorm2d in eval mode, i.e. a backward through `model.eval()`'s forward): coef is written as zeros, so that the apply
 * gives dx = gamma*invstd * dz; dgamma / dbeta are the same two sums. */
#define DSNT_BN_FROZEN 2
int dsnt_bn_act_bwd_reduce(const float* da, const float* x, const float* scale,
                           const float* shift, const float* mean, const float* invstd,
                           int relu, float* partial, int64_t M, int C, void* stream);
/* ... of y = relu?(bn(x) + skip) (`out = relu(bn2(conv2(..)) + identity)`, the tail of a torchvision BasicBlock / Bottleneck): the ReLU
 * mask is taken from the stored y, dz = da * (y > 0) is written (the skip branch's gradient and the apply read it) and the same tile sums
 * are left — dsnt_relu_bwd + dsnt_bn_act_bwd_reduce in one pass. */
int dsnt_bn_add_act_bwd_reduce(const float* da, const float* y, const float* x, const float* mean, const float* invstd,
                               int relu, float* dz, float* partial, int64_t M, int C, void* stream);
int dsnt_bn_bwd_finalize(const float* partial, int ntiles, int64_t M, int C,
                         float* dgamma, float* dbeta, int accumulate, float* coef,
                         void* stream);
/* The same, and the bound of dx = scale (dz - coef0 - xhat coef1) for dsnt_conv1x1_bwd_f16x3, which forms dx in registers and
 * needs its fp16x3 scale beforehand: max_c |scale_c| (max|dz| + |coef0_c| + |coef1_c| sqrt(M)) raised into bound_out (64 slots,
 * zeroed by the caller once per step); scale = the BatchNorm's forward scale (gamma * invstd), dz_amax = the 64-slot max |dz| the
 * data-gradient launch left through dsnt_out_bounds.amax.  hourglass.py:21,36-37 (bn2 of a Bottleneck, backward). */
int dsnt_bn_bwd_finalize_bound(const float* partial, int ntiles, int64_t M, int C, float* dgamma, float* dbeta,
                               int accumulate, float* coef, const float* scale, const float* dz_amax, float* bound_out,
                               void* stream);
int dsnt_bn_act_bwd_apply(const float* da, const float* x, const float* scale,
                          const float* shift, const float* mean, const float* invstd,
                          const float* coef, int relu, float* dx, int accumulate,
                          int64_t M, int C, void* stream);
/* The same, additionally raising amax[0] (device scalar, zeroed by the caller at the start of the step: dsnt_fill_zero)
 * (64 bound slots, slot = workgroup index mod 64) to max |dx| with integer atomic maxima on the floats' bits (order-independent): the operand bound of the fp16x3
 * data / weight gradient kernels that consume dx. */
int dsnt_bn_act_bwd_apply_amax(const float* da, const float* x, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* coef, int relu, float* dx,
                               int accumulate, int64_t M, int C, float* amax, void* stream);
/* dsnt_bn_act_bwd_apply(_amax) with dsnt_bn_bwd_finalize folded into its prologue (same limits as dsnt_bn_prologue):
 * partial[ntiles][2][C] = (sum dz, sum dz * xhat) tiles; coef is scratch of 2 * C floats the launch fills and reads;
 * dgamma / dbeta are written (+= with accumulate_params) by workgroup 0. */
int dsnt_bn_act_bwd_apply_pro(const float* da, const float* x, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const float* partial, int ntiles,
                              float* dgamma, float* dbeta, int accumulate_params, float* coef, int relu,
                              float* dx, int accumulate, int64_t M, int C, float* amax, void* stream);
/* Both with the result added to a tensor of its OWN instead of accumulated in place: dx = base + value, `base` read and never
 * written (amax may be NULL).  The gradient that dx continues — dL/d(block output) of a Bottleneck, hourglass.py:48 `out += residual`
 * — stays intact for a reader that comes later: the weight gradient of the block's conv3 then waits for its parameter bucket's grouped
 * launch like the other low-resolution weight gradients, instead of costing the dependency chain a launch of 2..32 workgroups. */
int dsnt_bn_act_bwd_apply_base(const float* da, const float* x, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* coef, int relu,
                               const float* base, float* dx, int64_t M, int C, float* amax, void* stream);
int dsnt_bn_act_bwd_apply_pro_base(const float* da, const float* x, const float* scale, const float* shift,
                                   const float* mean, const float* invstd, const float* partial, int ntiles,
                                   float* dgamma, float* dbeta, int accumulate_params, float* coef, int relu,
                                   const float* base, float* dx, int64_t M, int C, float* amax, void* stream);
int dsnt_fill_zero(float* p, int64_t n, void* stream);
/* The other kernels that (re)write a whole gradient tensor, with the same amax side output: a tensor written by several
 * of them in turn is bounded by the maximum over their amaxes (each rewrites all of it), so gradients accumulated along
 * the residual stream keep a valid fp16x3 bound. */
int dsnt_axpy_amax(const float* x, float* y, float a, int accumulate, int64_t n, float* amax, void* stream);
int dsnt_maxpool2_bwd_amax(const float* dy, const uint8_t* idx, float* dx, int accumulate, int N, int H, int W, int C,
                           float* amax, void* stream);
/* ... with a SECOND gradient of x added in the same pass: dx (+)= extra + the routed dy (amax may be NULL).  The hourglass's
 * stack input (hourglass.py:66-77: `up1 = self.hg[n-1][0](x)`, `low1 = F.max_pool2d(x, 2)` — and x also feeds the residual sum of
 * hourglass.py:175) collects three gradients; the skip branch's arrives in a buffer of its own, and this launch adds it instead of a
 * separate x.grad += branch.grad pass. */
int dsnt_maxpool2_bwd_add(const float* dy, const uint8_t* idx, float* dx, int accumulate, const float* extra,
                          int N, int H, int W, int C, float* amax, void* stream);
int dsnt_upsample2_bwd_amax(const float* dout, float* dlow, int accumulate, int N, int H, int W, int C, float* amax,
                            void* stream);

/* F.max_pool2d(x, 2, stride=2) (hourglass.py:80,111,162): y [N][H/2][W/2][C],
 * idx = position (0..3) of the first maximum in scan order, for the backward. */
int dsnt_maxpool2_fwd(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C,
                      void* stream);
int dsnt_maxpool2_bwd(const float* dy, const uint8_t* idx, float* dx, int accumulate,
                      int N, int H, int W, int C, void* stream);

/* ResNet pieces (torchvision resnet consumed by model.py:79-136; third-party, restated):
 * F.max_pool2d(x, 3, stride=2, padding=1): y [N][(H-1)/2+1][(W-1)/2+1][C], idx = winning tap 0..8;
 * y = relu?(scale*x + shift + res) (block tail: bn -> += identity -> relu); dz = dy * [y > 0];
 * zero-stuffing of dy for the data gradient of a strided convolution: out[n][oh*s][ow*s][c] = dy[n][oh][ow][c]. */
int dsnt_maxpool3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int dsnt_maxpool3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int accumulate, int N, int H, int W,
                        int C, void* stream);
int dsnt_bn_add_act_fwd(const float* x, const float* scale, const float* shift, const float* res, int relu,
                        float* y, int64_t M, int C, void* stream);
int dsnt_relu_bwd(const float* dy, const float* y, float* dz, int64_t n, void* stream);
int dsnt_zero_insert(const float* dy, float* out, int N, int Ho, int Wo, int C, int Hs, int Ws, int stride,
                     void* stream);

/* Data gradient of a STRIDED convolution, native (csrc/dgrad_up.hip): dx [N][H][W][Cin] (+= when res1 == dx) from
 * dy [N][Ho][Wo][Cout] and wd = dsnt_conv_pack_dgrad(w) ([Cin][R][S][Cout], taps flipped), g = the FORWARD convolution
 * (2 <= stride <= 4, Cout % 16 == 0: ask dsnt_conv_dgrad_strided_ok).  The pixels of dx are computed phase by phase
 * ((ih % stride, iw % stride): a 3x3 / 2 convolution has phases of 1, 2, 2 and 4 taps), so neither the zero-stuffed
 * copy of dy nor the multiplications by its zeros exist: 1 / stride^2 of the work of dsnt_zero_insert + dsnt_conv_fwd,
 * which it replaces in the engine.  Exact fp32 (v_mfma_f32_32x32x2_f32).  Optional epilogues, as dsnt_conv_fwd_ex:
 * res1 (may alias dx), or bnb + stats_partial ([dsnt_conv_dgrad_strided_tiles(g)][2][Cin], every row written),
 * or tail->amax (the other dsnt_out_bounds fields must be unset).  Replaces cuDNN's backward-data of the torchvision ResNet
 * stride-2 convolutions (conv1, layerN[0].conv1 / .conv2, downsample[0]) consumed by /root/reference/src/dsnt/model.py:103-121. */
int dsnt_conv_dgrad_strided(const float* dy, const float* wd, float* dx, const float* res1, float* stats_partial,
                            const dsnt_conv_geom* g, const dsnt_bn_bwd_epilogue* bnb, const dsnt_out_bounds* tail, void* stream);
int dsnt_conv_dgrad_strided_ok(const dsnt_conv_geom* g);
int dsnt_conv_dgrad_strided_tiles(const dsnt_conv_geom* g);

/* out = up + nearest_upsample2x(low) (hourglass.py:58,88-89); low [N][H/2][W/2][C]. */
int dsnt_upsample2_add_fwd(const float* up, const float* low, float* out,
                           int N, int H, int W, int C, void* stream);
/* dlow (+)= 2x2 block sums of dout. */
int dsnt_upsample2_bwd(const float* dout, float* dlow, int accumulate,
                       int N, int H, int W, int C, void* stream);

/* The same two forward ops with the BatchNorm statistics of their output in the same pass (the next op of the
 * hourglass is a BatchNorm: hourglass.py:33,78-90): partial[ceil(M/128)][2][C] exactly as dsnt_bn_stats over the
 * stored result would give (bit-identical), M = output pixels.  partial may be NULL (eval mode: no statistics;
 * tail->amax / amax_bn can still ask for the next convolution's fp16x3 operand bound). */
int dsnt_maxpool2_fwd_stats(const float* x, float* y, uint8_t* idx, float* partial, int N, int H, int W, int C,
                            const dsnt_out_bounds* tail, void* stream);
int dsnt_upsample2_add_fwd_stats(const float* up, const float* low, float* out, float* partial, int N, int H, int W,
                                 int C, const dsnt_out_bounds* tail, void* stream);
/* y = relu?(x * scale + shift) (dsnt_bn_act_fwd: the stem's materialised BatchNorm + ReLU, hourglass.py:157-159) with the
 * statistics of y in the same pass — the first Bottleneck's BatchNorm reads y next — and, through tail->amax / amax_bn, the
 * fp16x3 bound of the skip projection that reads y raw.  partial: [ceil(M/128)][2][C], may be NULL. */
int dsnt_bn_act_fwd_stats(const float* x, const float* scale, const float* shift, int relu, float* y, float* partial,
                          int64_t M, int C, const dsnt_out_bounds* tail, void* stream);

/* The 7x7 / stride 2 / pad 3 stem convolution on a C <= 4 channel image (hourglass.py:106; torchvision resnet conv1) as a
 * 4x4 / stride 1 / pad 1 convolution: dsnt_s2d_input writes the image as [N][H/2+1][W/2+1][16] (2x2 pixel blocks -> 16 channels,
 * one zero block row / column in front; tail->amax, if given, receives max|image| as the fp16x3 operand bound);
 * dsnt_s2d_weights re-packs OHWI [Cout][7][7][4] weights into [Cout][4][4][16] (back = 0) or gathers a [Cout][4][4][16] weight
 * gradient back into [Cout][7][7][4] (back = 1).  Any convolution entry point then runs the stem with K = 256. */
int dsnt_s2d_input(const float* src_nchw, float* dst, int N, int C, int H, int W, const dsnt_out_bounds* tail, void* stream);
int dsnt_s2d_weights(const float* w, float* w2, int Cout, int back, void* stream);
/* dsnt_s2d_weights (back = 0) + the filter's maximum (bound[64]) + its two fp16 planes (scaled as dsnt_split_f16x2 does,
 * plane stride Cout*256) + its three bf16 planes (dsnt_split_bf16x3 layout) in one launch; w2 (fp32 copy) may be NULL. */
int dsnt_s2d_weights_prep(const float* w, float* w2, void* planes16, void* planes_bf16, float* bound, int Cout, void* stream);

/* y (+)= a*x, flat; n % 4 == 0 not required. */
int dsnt_axpy(const float* x, float* y, float a, int accumulate, int64_t n, void* stream);

/* Layout changes at the model boundary (logical NCHW surface, model.py:229-231,
 * tests/test_model.py:22-23): src [N][C][HW] -> dst [N][HW][Cpad] (zero-filled pad)
 * and back (dst [N][C][HW] <- src [N][HW][Cpad]). */
int dsnt_nchw_to_nhwc(const float* src, float* dst, int N, int C, int HW, int Cpad, void* stream);
int dsnt_nhwc_to_nchw(const float* src, float* dst, int N, int C, int HW, int Cpad, void* stream);

/* ------------------------------------------------------------------ optimiser
 * train.py:314-326 — flat multi-tensor updates over the whole parameter arena. */
int dsnt_rmsprop_step(float* p, const float* g, float* square_avg, int64_t n, float lr,
                      float alpha, float eps, float weight_decay, float grad_scale, void* stream);
int dsnt_sgd_step(float* p, const float* g, float* momentum_buf, int64_t n, float lr,
                  float momentum, float weight_decay, float grad_scale, int first_step,
                  void* stream);
/* The same updates under the step's non-finite guard (train.py:360-371 checks the loss for NaN before
 * `backward()` / `step()` and dumps the model): `flag` is a device int[2] the caller owns and zeroes.  If
 * flag[0] != 0 when the kernel starts (the loss check below fired earlier on this stream) NOTHING is updated — the
 * weights stay the last finite ones; an element whose own gradient is not finite is skipped and raises
 * DSNT_FLAG_GRAD in flag[1], which the next dsnt_nonfinite_flag call promotes into flag[0]. */
#define DSNT_FLAG_LOSS 1
#define DSNT_FLAG_GRAD 2
int dsnt_rmsprop_step_guarded(float* p, const float* g, float* square_avg, int64_t n, float lr, float alpha,
                              float eps, float weight_decay, float grad_scale, int* flag, void* stream);
int dsnt_sgd_step_guarded(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum,
                          float weight_decay, float grad_scale, int first_step, int* flag, void* stream);
/* flag[0] |= code if any of x[0..n) is NaN or +-inf (train.py:360 `np.isnan(loss.data[0])`, without the
 * device-to-host synchronisation: the caller reads the flag asynchronously); also flag[0] |= flag[1]. */
int dsnt_nonfinite_flag(const float* x, int64_t n, int* flag, int code, void* stream);

/* ------------------------------------------------------------------ launch lists
 * The reference re-records its autograd graph and issues ~10^3 device ops from Python every step (train.py:355-384).
 * Here a step is a fixed sequence of the entry points above; a launch list captures that sequence ONCE and replays it
 * from C: between dsnt_list_begin and dsnt_list_end (per thread) every entry point validates its arguments as usual but
 * records its kernel launches (arguments by value) instead of enqueueing them, and its `stream` argument is read as a
 * LANE index 0..DSNT_MAX_LANES-1.  dsnt_list_sync appends "lane dst waits for everything lane src has been given so
 * far" (an event the list owns); dsnt_list_mark ends a segment (the caller does host work there — e.g. starts an
 * all-reduce — between replays) and returns the index of the segment that begins.  dsnt_list_replay enqueues one
 * segment (-1: all) on the caller's streams, lane i -> streams[i].  A list holds pointers, not memory: the caller keeps
 * every tensor it recorded alive and unchanged in address.  dsnt_amax (memset) cannot be recorded. */
#define DSNT_MAX_LANES 8
typedef struct dsnt_list dsnt_list;
dsnt_list* dsnt_list_create(void);
void dsnt_list_destroy(dsnt_list* l);
int dsnt_list_begin(dsnt_list* l);
int dsnt_list_end(void);
int dsnt_list_sync(dsnt_list* l, int src_lane, int dst_lane);
int dsnt_list_mark(dsnt_list* l);
int dsnt_list_segments(const dsnt_list* l);
int dsnt_list_size(const dsnt_list* l);
int dsnt_list_replay(const dsnt_list* l, int segment, void* const* streams, int nstreams);

/* ------------------------------------------------------------------ metrics
 * evaluator.py:66-81 + train.py:243-258: PCKh hits on device.
 * pred/target [B][J][2] normalised coords; m [B][2][2], b [B][2] back-projection (f64 maths);
 * mask [B][J]; head [B]; out hits[B][J] (1/0), valid[B][J] (mask == 1). */
int dsnt_pckh(const float* pred, const float* target, const double* m, const double* b,
              const float* mask, const double* head, float threshold, float* hits,
              float* valid, int B, int J, void* stream);
/* evaluator.py:66-81 + train.py:243-258 for a whole PCKh curve: one launch ADDS a batch to a histogram of the normalised
 * distance per joint, whose bin edges are the thresholds.  d is dsnt_pckh's distance (same fp64 expression); a joint
 * with mask == 1 adds 1 to table[j][k], k the smallest index with d <= thresholds[k], or to table[j][T] when there is
 * none (d beyond the last threshold, NaN, inf from a zero head length); other masks add nothing.  Hits at thresholds[k]
 * are sum(table[j][0..k]), the valid count is the row sum.
 * thresholds: HOST double[T], 1 <= T <= DSNT_PCKH_HIST_MAX_T, finite and strictly ascending, passed by value to the
 * kernel (DSNT_ERR_ARG otherwise, nothing launched).  table: device u64 [J][T + 1]; the kernel only adds (64-bit integer
 * atomics: order-independent, bit-reproducible), the caller zeroes.  dist (may be NULL): device f64 [B][J] = d where
 * mask == 1, NaN elsewhere.
 * The grid is min(ceil(B * J / DSNT_PCKH_HIST_BLOCK), DSNT_PCKH_HIST_MAX_BLOCKS) workgroups striding over B * J.  While
 * J * (T + 1) <= DSNT_PCKH_HIST_LDS_CELLS each workgroup counts in LDS and flushes its non-zero cells once; above that
 * every joint adds to `table` directly.  dsnt_version() >= 122. */
#define DSNT_PCKH_HIST_MAX_T 64
#define DSNT_PCKH_HIST_LDS_CELLS 4096
#define DSNT_PCKH_HIST_BLOCK 256
#define DSNT_PCKH_HIST_MAX_BLOCKS 64
int dsnt_pckh_hist(const float* pred, const float* target, const double* m, const double* b,
                   const float* mask, const double* head, const double* thresholds, int T,
                   unsigned long long* table, double* dist, int B, int J, void* stream);
/* bin/investigate.py:62-99, the misprediction field: one launch ADDS a batch to a bins x bins grid per joint over the
 * normalised location of the TARGET, holding how many joints lay in each cell, how many of them missed, and the summed
 * offset of the misses.  pred, target, m, b, mask, head and threshold are dsnt_pckh's, d is its distance (same fp64
 * expression), and a joint is a miss here exactly when dsnt_pckh gives it no hit: !(d <= threshold), so a NaN or inf d
 * (zero head length, non-finite prediction) is a miss.
 * A joint counts only if mask == 1 and edges[0] <= tx <= edges[bins] and likewise ty (tx, ty: the fp32 target widened to
 * fp64; a NaN target fails the comparison).  Its cell along an axis is the number of edges[1..bins] that are <= t, capped
 * at bins - 1: e_k <= t < e_{k+1} with the last edge closed, which is scipy.stats.binned_statistic_dd(range=...).  Then
 * total[j][cy][cx] += 1; on a miss, miss += 1 and, with dx = (double)px - tx and dy likewise, if both are finite:
 * miss_finite += 1, sum_x += dx, sum_y += dy (a non-finite prediction is counted and kept out of the sums).
 * edges: HOST double[bins + 1], 1 <= bins <= DSNT_ERROR_FIELD_MAX_BINS, finite and strictly ascending, the same for x
 * and y, passed by value to the kernel (DSNT_ERR_ARG otherwise, nothing launched).  counts: device i64
 * [3][J][bins][bins], planes total, miss, miss_finite, cells [by][bx]; sums: device f64 [2][J][bins][bins], planes sum
 * of dx and of dy.  The kernel only adds to both; the caller zeroes.
 * No atomics: the grid is J workgroups of DSNT_ERROR_FIELD_BLOCK threads, workgroup j owns joint j and lane l of it owns
 * the cells l, l + DSNT_ERROR_FIELD_BLOCK, ...; the lane loads the sums' current values, adds its samples in ascending n
 * and stores.  The tables are therefore bit-identical to a sequential loop over n, and the same whether a set arrives as
 * one batch or as several.  dsnt_version() >= 124. */
#define DSNT_ERROR_FIELD_MAX_BINS 32
#define DSNT_ERROR_FIELD_BLOCK 256
int dsnt_error_field(const float* pred, const float* target, const double* m, const double* b,
                     const float* mask, const double* head, float threshold,
                     const double* edges, int bins, int64_t* counts, double* sums,
                     int B, int J, void* stream);
/* Does the confidence know?  One launch ADDS a batch to a two-way histogram per joint: the score of a joint (any per-joint
 * statistic, e.g. the heat-map's peak) against its normalised distance.  pred, target, m, b, mask, head, thresholds and T
 * are dsnt_pckh_hist's, with the same checks; d is dsnt_pckh's distance (same fp64 expression) and the column k is
 * dsnt_pckh_hist's: the smallest index with d <= thresholds[k], or T when there is none (beyond the last threshold, NaN,
 * inf).  score: device f32 [B][J].  The row r is the number of score_edges that are <= the score widened to fp64: row 0 is
 * score < e[0], row S is score >= e[S - 1], a score equal to an edge goes to the upper row, -inf to row 0, +inf to row S;
 * a NaN score goes to row S + 1, the "unscored" row.  A joint with mask == 1 adds 1 to table[j][r][k]; other masks add
 * nothing.  Summed over r the table is dsnt_pckh_hist's, bit for bit.
 * score_edges: HOST double[S], 1 <= S <= DSNT_SCORE_HIST_MAX_S, finite and strictly ascending, passed by value to the
 * kernel and padded with +inf, as the thresholds are (DSNT_ERR_ARG otherwise, nothing launched).  table: device u64
 * [J][S + 2][T + 1]; the kernel only adds (64-bit integer atomics: order-independent, bit-reproducible), the caller zeroes.
 * The grid and striding are dsnt_pckh_hist's.  While J * (S + 2) * (T + 1) <= DSNT_SCORE_HIST_LDS_CELLS each workgroup
 * counts in a u32 LDS copy of the table and flushes its non-zero cells with one 64-bit atomic each; above that every joint
 * adds to `table` directly.  dsnt_version() >= 126. */
#define DSNT_SCORE_HIST_MAX_S 64
#define DSNT_SCORE_HIST_LDS_CELLS 8192
int dsnt_score_hist(const float* pred, const float* target, const double* m, const double* b,
                    const float* mask, const double* head, const float* score,
                    const double* score_edges, int S, const double* thresholds, int T,
                    unsigned long long* table, int B, int J, void* stream);
/* The table read back as a function of the score: out[i] = values[(per_joint ? i % J : 0) * (S + 2) + row(score[i])] for
 * i in 0..n-1, row being dsnt_score_hist's rule (NaN scores read row S + 1).  score, out: device f32 [n] (n = B * J with
 * per_joint); values: device f32 [J][S + 2], or [1][S + 2] when per_joint == 0; NaN entries pass through.  score_edges as
 * above.  per_joint is 0 or 1, n >= 1, J >= 1 (DSNT_ERR_ARG otherwise, nothing launched).  Plain stores; the grid is
 * min(ceil(n / DSNT_SCORE_LOOKUP_BLOCK), DSNT_SCORE_LOOKUP_MAX_BLOCKS) workgroups striding over n.
 * dsnt_version() >= 126. */
#define DSNT_SCORE_LOOKUP_BLOCK 256
#define DSNT_SCORE_LOOKUP_MAX_BLOCKS 1024
int dsnt_score_lookup(const float* score, const double* score_edges, int S, const float* values,
                      int per_joint, float* out, int64_t n, int J, void* stream);
/* How far can a PCKh be trusted?  One launch ADDS a batch to R + 1 copies of dsnt_pckh_hist's table: copy 0 counts every
 * example once, copy r in 1..R counts example n w(ids[n], r) times, a Poisson(1) bootstrap over examples (people: all the
 * joints of an example share its weight).  pred, target, m, b, mask, head, thresholds and T are dsnt_pckh_hist's, with the
 * same checks; d is dsnt_pckh's distance (same fp64 expression) and the column k is dsnt_pckh_hist's.  A joint with
 * mask == 1 adds w(ids[n], r) to table[r][j][k] for every r in 0..R; other masks add nothing.  table[0] is
 * dsnt_pckh_hist's table bit for bit.
 * The weight.  w(id, 0) = 1.  For r in 1..R: u = word (r - 1) & 3 of Philox4x32-10 with key (seed lo, seed hi) and counter
 * (id lo, id hi, (r - 1) >> 2, DSNT_PCKH_BOOT_DOMAIN), id being the int64 taken as its 64 bits (one Philox call serves four
 * replicates; the domain word keeps the stream apart from the augmentation draw's 0, 1, 2 and the epoch order's
 * 0x4F524400 + i), and w = the number of k in 0..11 with u >= c_k, c_k = floor(2^32 e^-1 sum_{i<=k} 1/i!) as listed in
 * DSNT_PCKH_BOOT_CDF: the inverse CDF of Poisson(1) on 32 bits, w in 0..12, mean 1 + 2e-9.  The weight depends on the
 * example's id, the replicate and the seed alone: not on the batch, its order or the rank that holds it, and two models
 * fed the same ids resample the same people.
 * ids: device i64 [B], any values.  table: device u64 [R + 1][J][T + 1]; the kernel only adds (64-bit integer atomics:
 * order-independent, bit-reproducible), the caller zeroes.  R >= 1 and (R + 1) * J * (T + 1) fits an int.
 * B <= DSNT_PCKH_BOOT_MAX_B = floor((2^32 - 1) / 12): a workgroup counts in 32 bits on chip, and one cell takes at most
 * 12 from each of the at most B examples the workgroup sees.  DSNT_ERR_ARG otherwise, nothing launched.
 * A workgroup of DSNT_PCKH_BOOT_BLOCK threads owns a chunk of min(DSNT_PCKH_BOOT_CHUNK, DSNT_PCKH_BOOT_LDS_CELLS /
 * (J * (T + 1))) consecutive copies; grid.x = min(chunks, DSNT_PCKH_BOOT_MAX_CHUNK_BLOCKS) strides over the chunks.  It
 * walks B * J in spans of DSNT_PCKH_BOOT_SPAN joints (grid.y = min(spans, DSNT_PCKH_BOOT_MAX_SPAN_BLOCKS) strides over
 * them): the column of every joint of the span once, into LDS, then one thread per (example, four replicates).  While
 * J * (T + 1) <= DSNT_PCKH_BOOT_LDS_CELLS the chunk is summed in a u32 LDS table and its non-zero cells are flushed with
 * one 64-bit atomic each; above that every weight is added to `table` directly.  dsnt_version() >= 127. */
#define DSNT_PCKH_BOOT_DOMAIN 0x424F4F54u
#define DSNT_PCKH_BOOT_CDF { 1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u, 4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u }
#define DSNT_PCKH_BOOT_MAX_B 357913941
#define DSNT_PCKH_BOOT_LDS_CELLS 4096
#define DSNT_PCKH_BOOT_BLOCK 256
#define DSNT_PCKH_BOOT_CHUNK 32
#define DSNT_PCKH_BOOT_SPAN 1024
#define DSNT_PCKH_BOOT_MAX_CHUNK_BLOCKS 1024
#define DSNT_PCKH_BOOT_MAX_SPAN_BLOCKS 16
int dsnt_pckh_boot(const float* pred, const float* target, const double* m, const double* b,
                   const float* mask, const double* head, const int64_t* ids,
                   const double* thresholds, int T, uint64_t seed, int R,
                   unsigned long long* table, int B, int J, void* stream);
/* What kind of miss was it?  One launch ADDS a batch to a joint-confusion table: which joint of the same person a
 * prediction landed on.  pred, target, m, b, mask, head and threshold are dsnt_pckh's.  With P_j the back-projected
 * prediction of a counted joint j (mask[n][j] == 1), G_k the back-projected target of every annotated joint k of the same
 * person (mask[n][k] == 1), d_jk = |P_j - G_k| / head[n] (dsnt_pckh's fp64 expression, which d_jj is) and t the threshold
 * widened to fp64, the joint adds 1 to exactly one cell of table[j]:
 *   d_jj <= t: column j, the very hit dsnt_pckh counts;
 *   otherwise column k, the annotated k != j of smallest d_jk among those with d_jk <= t (an exact tie goes to the
 *   smallest k);
 *   otherwise column J: it landed on no annotated joint.  A NaN prediction ends here, as does an inf or NaN d from a zero
 *   head length: no comparison holds.
 * A joint that is not counted adds nothing, and a target that is not annotated attracts nothing: its coordinates may be
 * NaN.  The row sums are dsnt_pckh's valid counts and the diagonal its hits.
 * mirror: HOST int[J], an involution of 0..J-1 (mirror[mirror[j]] == j; mirror[j] == j: no partner), checked on the host
 * and passed by value to the kernel, never read from device memory.  For m = mirror[j] != j, mutual[j] gets 1 when the
 * cell of j is column m, m is counted and the cell of m is column j: the pair was exchanged, which a collapse of both
 * onto one target is not.  mutual[j] == mutual[mirror[j]] always.
 * table: device u64 [J][J + 1], mutual: device u64 [J]; the kernel only adds (64-bit integer atomics: order-independent,
 * bit-reproducible, the same however the examples are batched), the caller zeroes.
 * DSNT_ERR_ARG and nothing launched for, in this order: a null pointer, B <= 0, J outside 1..DSNT_CONFUSION_MAX_J, a
 * threshold that is negative or not finite, a mirror that is not an involution (the message names the first j with
 * mirror[j] outside 0..J-1 or mirror[mirror[j]] != j).
 * The unit of work is the person: min(ceil(B / per), DSNT_CONFUSION_MAX_BLOCKS) workgroups of DSNT_CONFUSION_BLOCK
 * threads stride over the persons, per = DSNT_CONFUSION_BLOCK / J at a time; the J targets of a person are back-projected
 * once, into LDS.  Each workgroup counts in a u32 LDS copy [J][J + 2] (table, then mutual) and flushes its non-zero cells
 * with one 64-bit atomic each.  dsnt_version() >= 128. */
#define DSNT_CONFUSION_MAX_J 64
#define DSNT_CONFUSION_BLOCK 256
#define DSNT_CONFUSION_MAX_BLOCKS 64
int dsnt_joint_confusion(const float* pred, const float* target, const double* m, const double* b,
                         const float* mask, const double* head, float threshold, const int* mirror,
                         unsigned long long* table, unsigned long long* mutual, int B, int J, void* stream);
/* Was the heat-map right and the read-out wrong?  The mass of a joint's heat-map that lies within the threshold of the
 * truth, and of the mirrored joint's truth.  heatmaps: device f32 [B][J][h][w]; target, m, b, mask, head, threshold and
 * mirror are dsnt_joint_confusion's.  The centre of pixel (r, c) has the normalised coordinates x = (2c + 1 - w) / w,
 * y = (2r + 1 - h) / h (fp64; dsnt.nn.generate_xy's grid); it is back-projected as a prediction is, and its distance to a
 * target in head lengths is dsnt_pckh's expression with these fp64 coordinates in place of the prediction's.
 * out: device f32 [B][J][2].  For a counted joint (mask[n][j] == 1) out[n][j][0] = the sum of hm[n][j] over the pixels
 * within the threshold of G_j, and out[n][j][1] the same round G_mirror[j], or NaN when mirror[j] == j or the mirror joint
 * is not annotated; both are NaN when the joint is not counted.  The sums are of the values as given: probabilities only
 * for a normalised map.  0 when the disc holds no pixel centre.
 * Summed in fp64 in a fixed order and rounded to f32 once: bit-reproducible, and the same for any alignment of
 * `heatmaps`.  One workgroup of DSNT_TARGET_MASS_BLOCK threads per (n, j); thread t takes the pixels 4q .. 4q + 3 of the
 * flat map for q = t, t + DSNT_TARGET_MASS_BLOCK, ... (one 16-byte load each when w % 4 == 0 and heatmaps is 16-byte
 * aligned, scalar loads otherwise), then a xor tree across each wave and the waves in ascending order.  Every pixel is
 * tested and the map is read once.
 * Refuses what dsnt_joint_confusion refuses, with its own name in the message, then B * J >= 2^31 (DSNT_ERR_ARG) and maps
 * dsnt_heatmap_stats refuses: h, w > 0 and h * w < 2^24 (DSNT_ERR_SHAPE).  dsnt_version() >= 128. */
#define DSNT_TARGET_MASS_BLOCK 256
int dsnt_target_mass(const float* heatmaps, const float* target, const double* m, const double* b,
                     const float* mask, const double* head, float threshold, const int* mirror, float* out,
                     int B, int J, int h, int w, void* stream);
/* Mode-seeking read-out: the K dominant modes of each heat-map as window centroids (csrc/modes.hip).
 * hm: device f32 [rows][h][w], one map p per row, used as given (nothing is normalised); rows = B J, sample b = row / J.
 * radius r in map pixels, 0..DSNT_MODES_MAX_RADIUS; K modes, 1..DSNT_MODES_MAX_K.
 * Window score S[y][x] = the sum of p over the (2r+1)^2 window centred on (y, x), clipped to the map, in fp32 in this
 * order: s[y][x] = sum_{d=-r..r} p[y][x+d] in ascending d from +0, a pixel outside the map adding +0, then
 * S[y][x] = sum_{d=-r..r} s[y+d][x] by the same rule; every add is rounded separately (no sliding window).
 * Mode 0 is the centre with the largest S: scanning in row-major order from best = -inf a candidate wins only if
 * S > best, so an exact tie goes to the smallest index y w + x, a NaN S never wins, and a row without a winner has index
 * -1.  Mode k > 0 is chosen the same way among the centres whose Chebyshev distance from every earlier mode's centre
 * exceeds 2r (its window is disjoint from theirs); -1 when there is none.
 * Per mode, with the sums over its clipped window in fp64 (per window row in ascending x from +0, then the rows in
 * ascending y from +0; X p and Y p rounded before they are added) on the grid X = (2x+1)/w - 1, Y = (2y+1)/h - 1 (fp64):
 *   index  i32 [rows][K]     the centre y w + x, or -1
 *   mass   f32 [rows][K]     (float) sum p
 *   coords f32 [rows][K][2]  (float)(sum X p / sum p), (float)(sum Y p / sum p)
 *   image  f64 [rows][K][2]  transform_b[b] + coords . transform_m[b] on row vectors (dsnt_flip_merge_head's convention),
 *                            from the f32-rounded coordinates; transform_m f64 [B][2][2], transform_b f64 [B][2].
 *                            Optional: transform_m, transform_b and image are all NULL or all non-NULL.
 * When sum p is not > 0, coords and image are NaN and mass is as computed; for index -1 mass, coords and image are NaN.
 * One workgroup of 256 threads per row, the row and its row sums in two LDS planes (h w <= DSNT_MODES_MAX_PIXELS: 64 KiB);
 * plain stores, no atomics: bit-reproducible, and the same for any alignment of hm (16-byte loads when w % 4 == 0 and hm
 * is 16-byte aligned, scalar loads otherwise).
 * Refused, nothing launched, in this order: a null hm, coords, mass or index; rows outside 1..2^31-1, J < 1 or
 * rows % J != 0; radius; K; inconsistent optional pointers (DSNT_ERR_ARG); h, w < 1 or h w > DSNT_MODES_MAX_PIXELS
 * (DSNT_ERR_SHAPE: dsnt_heatmap_stats takes larger maps).  dsnt_version() >= 129. */
#define DSNT_MODES_MAX_RADIUS 8
#define DSNT_MODES_MAX_K 4
#define DSNT_MODES_MAX_PIXELS 8192
int dsnt_map_modes(const float* hm, int64_t rows, int J, int h, int w, int radius, int K,
                   const double* transform_m, const double* transform_b,
                   float* coords, float* mass, int* index, double* image, void* stream);

/* ------------------------------------------------------------------ training augmentation
 * data.py:118-226 (MPIIDataset.__getitem__, use_aug) batched on the device; semantics in csrc/augment.hip.
 * dsnt_augment_fwd: src uint8 [B][R][R][3] (HWC crops) -> out f32 [B][3][S][S] = normalize(adaptive_avg_pool(clamp(gain *
 * center_crop(rotate(flip(src)), int(R*scale)) / 255))).  Per-sample parameters scale [B], rot_deg [B], hflip [B] (0/1),
 * gain [B][3]; mean, stdv [3] (device).  draw != 0: the parameters are first drawn on the device from Philox(seed; sample,
 * step) with the reference's distributions (data.py:134-140, 205-210) and written to those four buffers; draw == 0: they are
 * read.  R <= 8192, S <= 4096, B <= 65535.  Bit-reproducible (no atomics).  dsnt_version() >= 115 (all three entry points). */
int dsnt_augment_fwd(const uint8_t* src, int B, int R, int S, float* scale, float* rot_deg, uint8_t* hflip,
                     float* gain, int draw, uint64_t seed, uint64_t step, const float* mean, const float* stdv,
                     float* out, void* stream);
/* dsnt_augment_fwd_pair: dsnt_augment_fwd with out f32 [2B][3][S][S]; out[B + b][c][y][x] = out[b][c][y][S-1-x], the
 * mirrored twin flip test-time augmentation feeds the model (replaces inference.py:37's cat + reverse_tensor).
 * dsnt_version() >= 116. */
int dsnt_augment_fwd_pair(const uint8_t* src, int B, int R, int S, float* scale, float* rot_deg, uint8_t* hflip,
                          float* gain, int draw, uint64_t seed, uint64_t step, const float* mean, const float* stdv,
                          float* out, void* stream);
/* data.py:150-196 in fp64: matrix [B][3][3] (bb transform), keypoints [B][J][2] (original-image pixels), keypoint_mask
 * [B][J]; the parameters of dsnt_augment_fwd; flip_idx [J] (a permutation: inference.HFLIP_INDICES); train != 0: mask joints
 * with |coord| >= 1.  Out: part_coords f32 [B][J][2], part_mask f32 [B][J], trans_m f64 [B][2][2], trans_b f64 [B][1][2]. */
int dsnt_augment_keypoints(const double* matrix, const double* keypoints, const float* keypoint_mask, int B, int J,
                           const float* scale, const float* rot_deg, const uint8_t* hflip, const int64_t* flip_idx,
                           int train, float* part_coords, float* part_mask, double* trans_m, double* trans_b,
                           void* stream);
/* Gather variants for a device-resident training set (dsnt.data.DeviceDataset / EpochLoader).  dsnt_version() >= 118.
 * dsnt_augment_fwd_gather / _pair_gather: dsnt_augment_fwd / _pair where sample b is row idx[b] (int64 [B]) of pool uint8
 * [N][R][R][3], drawn (draw != 0) with Philox sample word b + draw_offset (0: exactly dsnt_augment_fwd's draw; rank r of W
 * passes r * B).  An index outside [0, N) reads nothing and makes that sample's input NaN. */
int dsnt_augment_fwd_gather(const uint8_t* pool, int64_t N, const int64_t* idx, int B, int R, int S, float* scale,
                            float* rot_deg, uint8_t* hflip, float* gain, int draw, uint64_t seed, uint64_t step,
                            uint32_t draw_offset, const float* mean, const float* stdv, float* out, void* stream);
int dsnt_augment_fwd_pair_gather(const uint8_t* pool, int64_t N, const int64_t* idx, int B, int R, int S, float* scale,
                                 float* rot_deg, uint8_t* hflip, float* gain, int draw, uint64_t seed, uint64_t step,
                                 uint32_t draw_offset, const float* mean, const float* stdv, float* out, void* stream);
/* dsnt_augment_keypoints on rows idx[b] of matrix_pool f64 [N][3][3], kp_pool f64 [N][J][2], mask_pool f32 [N][J]; also
 * writes normalize f64 [B] = head_len_pool[idx[b]] (f64 [N]).  An index outside [0, N) reads nothing: part_mask 0,
 * part_coords, trans_m, trans_b and normalize NaN. */
int dsnt_augment_keypoints_gather(const double* matrix_pool, const double* kp_pool, const float* mask_pool,
                                  const double* head_len_pool, int64_t N, const int64_t* idx, int B, int J,
                                  const float* scale, const float* rot_deg, const uint8_t* hflip, const int64_t* flip_idx,
                                  int train, float* part_coords, float* part_mask, double* trans_m, double* trans_b,
                                  double* normalize, void* stream);
/* out int64 [count] = order(first + i): a bijection of [0, n) keyed by (seed, epoch), an 8-round Feistel network of
 * Philox4x32-10 round functions over 2^k >= n with cycle-walking (construction in csrc/augment.hip); shuffle == 0: the
 * identity.  Needs 0 <= first, 0 < count <= n - first. */
int dsnt_epoch_indices(int64_t n, uint64_t seed, uint64_t epoch, int64_t first, int64_t count, int shuffle, int64_t* out,
                       void* stream);
/* Importance-sampled epochs (dsnt.data.ExampleScores / WeightedLoader; csrc/sampler.hip).  dsnt_version() >= 130.
 *
 * dsnt_sample_cdf: cdf u64 [n] = an exact fixed-point CDF of weights f32 [n], 1 <= n <= DSNT_SAMPLE_MAX_N.  A weight that
 * is NaN, +-inf, negative or zero counts as 0 (a positive subnormal counts).  wmax = the largest counted weight = f 2^e
 * with f in [0.5, 1) (frexp); q[i] = floor(w[i] 2^(32 - e)), an integer below 2^32 (scaling by a power of two is exact:
 * nothing is rounded); cdf[i] = q[0] + .. + q[i], below 2^56, so exact and independent of the order of summation.  The
 * resolution is 2^-32 of the binade of the largest weight: a weight below 2^(e - 32), i.e. less than about 2^-31 .. 2^-32
 * of the largest, has q = 0, and SUCH A ROW IS NEVER DRAWN, like a row of weight 0.  If no weight counts, cdf is all
 * zero.  scratch: DSNT_SAMPLE_CDF_SCRATCH_BYTES(n) bytes of device memory, 8-byte aligned, initialised by the call
 * (contents on return unspecified).  Five stream-ordered launches: zero the maximum; an integer atomic max over the bit
 * patterns of the counted weights (order-independent); a scan inside every tile of DSNT_SAMPLE_TILE weights; one
 * workgroup scans the tile totals; every tile adds its offset.  No workgroup waits on another workgroup of its launch.
 * Bit-reproducible.  DSNT_ERR_ARG: a null pointer; DSNT_ERR_SHAPE: n out of range; nothing launched. */
#define DSNT_SAMPLE_MAX_N (1 << 24)
#define DSNT_SAMPLE_TILE 1024
#define DSNT_SAMPLE_CDF_SCRATCH_BYTES(n) (8 * (1 + ((int64_t)(n) + DSNT_SAMPLE_TILE - 1) / DSNT_SAMPLE_TILE))
int dsnt_sample_cdf(const float* weights, int64_t n, uint64_t* cdf, void* scratch, void* stream);
/* out int64 [count] = the weighted draws, with replacement, of positions first .. first + count - 1 of an epoch from the
 * cdf u64 [n] of dsnt_sample_cdf (any non-decreasing u64 [n] serves).  Position p: (o0, o1, ., .) =
 * Philox4x32-10 with key (seed lo, seed hi) and counter (p, epoch lo, epoch hi, DSNT_SAMPLE_DOMAIN), a domain word apart
 * from the augmentation draw's 0, 1, 2, the epoch order's 0x4F524400 + 0..7 and DSNT_PCKH_BOOT_DOMAIN; u = o0 2^32 + o1;
 * T = cdf[n - 1]; t = floor(u T / 2^64); out = the smallest j with cdf[j] > t, so row j is drawn with probability q[j] / T
 * to within 2^-64.  T == 0: out = -1, which the gather kernels turn into a NaN sample with mask 0.  The draw depends on
 * (seed, epoch, p) alone: not on count, on the sub-range or on who asks.  One launch, one thread per position, a bisection
 * of ceil(log2 n) loads.  Needs 1 <= n <= DSNT_SAMPLE_MAX_N, 0 <= first, 0 < count, first + count <= 2^32 (DSNT_ERR_SHAPE
 * otherwise), non-null pointers (DSNT_ERR_ARG); nothing launched on an error. */
#define DSNT_SAMPLE_DOMAIN 0x57534D50u
int dsnt_sample_indices(const uint64_t* cdf, int64_t n, uint64_t seed, uint64_t epoch, int64_t first, int64_t count,
                        int64_t* out, void* stream);
/* Per-row error table.  pred .. head: dsnt_pckh's arguments; idx int64 [B]: the dataset row of each example.  score f32
 * [B] = the mean of dsnt_pckh's distance (same fp64 expression) over the joints of the example with mask == 1, summed in
 * fp64 in joint order, divided by their number and rounded to fp32; NaN with no such joint.  table u64 [N] (0 = never
 * seen): when score[b] is finite and 0 <= idx[b] < N, one 64-bit atomic max of (stamp << 32) | bits(score[b]) into
 * table[idx[b]]; nothing is written otherwise.  Head lengths are positive, so scores are non-negative and their bit order
 * is their order: the newest stamp wins, and within a stamp the larger score, whatever the order of arrival (a row drawn
 * twice in a batch is deterministic).  One thread per example: it is not a hot kernel.  DSNT_ERR_ARG and nothing
 * launched: a null pointer, B <= 0, J <= 0, N < 1, stamp outside [1, 2^31). */
int dsnt_example_scores(const float* pred, const float* target, const double* m, const double* b, const float* mask,
                        const double* head, const int64_t* idx, int64_t N, uint32_t stamp, unsigned long long* table,
                        float* score, int B, int J, void* stream);
/* Synthetic occlusion of a batch of model inputs (dsnt.data.Occlude; csrc/occlude.hip).  dsnt_version() >= 131.
 * in f32 [B][3][S][S] -> out f32 [B][3][S][S]: out = in outside the sample's rectangles (bits copied: NaN, infinities
 * and -0 pass through), the fill inside them.  One launch.  Out of place: the paste fill reads another sample of `in`,
 * which in place might already hold that sample's own occlusion; in == out or overlapping ranges: DSNT_ERR_ARG.
 * Small outputs: rects int32 [B][K][4] = (x0, y0, x1, y1), half-open, unused rows all zero; donor int32 [B]; occluded
 * uint8 [B][J] (J > 0) = 1 iff joint j's pixel lies in some rectangle of sample b, whatever its mask.  coords f32
 * [B][J][2] normalised; a joint's pixel is (int)floorf((c + 1.f) * (0.5f * S)) per coordinate in fp32; NaN or outside
 * [0, S): the joint has no pixel, centres nothing and is never covered.  mask f32 [B][J] is read by joint centring only.
 * draw != 0, integers only: u24(x) = x >> 8; pick(x, n) = (u24(x) * n) >> 24 in 64 bits; P(k) = the four words of
 * Philox4x32-10 with key (seed lo, seed hi) and counter (g, step lo, step hi, DSNT_OCCLUDE_DOMAIN + k), g = draw_offset
 * + b; the domain words DSNT_OCCLUDE_DOMAIN + 0..10 lie apart from the augmentation draw's 0, 1, 2, the epoch order's
 * 0x4F524400 + 0..7, DSNT_PCKH_BOOT_DOMAIN and DSNT_SAMPLE_DOMAIN.  A = P(0): occluded iff u24(A0) < p24 (the host passes
 * p24 = round(p 2^24) <= 2^24); count = 1 + pick(A1, K) if so, else 0; donor = (b + 1 + pick(A2, B - 1)) % B for B > 1,
 * else b.  Rectangle r < count, Rr = P(1 + r): w = side_min + pick(Rr0, side_max - side_min + 1), h likewise from Rr1;
 * centre DSNT_OCCLUDE_CENTRE_UNIFORM: cx = pick(Rr2, S), cy = pick(Rr3, S); DSNT_OCCLUDE_CENTRE_JOINT: with nv = the
 * number of joints with mask != 0 that have a pixel, nv > 0: the pixel of the pick(Rr2, nv)-th such joint in index
 * order, nv == 0: the uniform rule; x0 = max(cx - w/2, 0), x1 = min(cx - w/2 + w, S) (integer division), y alike.
 * draw == 0: rects and donor are inputs; the kernel clamps every coordinate into [0, S] and the donor into [0, B) (the
 * clamp is the contract: nothing a device tensor holds addresses outside the batch); x1 <= x0 or y1 <= y0 is empty.
 * Fills (overlapping rectangles agree by construction): DSNT_OCCLUDE_FILL_VALUE, channel c = fill_value[c];
 * DSNT_OCCLUDE_FILL_NOISE, Nw = P(9), ns = Nw0 | Nw1 << 32, pixel q = y S + x takes the words of Philox4x32-10 with key
 * ns and counter (q, step lo, step hi, DSNT_OCCLUDE_DOMAIN + 10), u = (float)(u24(word c) + 1) * 2^-24 (exact), value =
 * (u - mean[c]) / stdv[c], each step rounded to fp32; DSNT_OCCLUDE_FILL_PASTE, the pixel of sample donor at the same
 * position of `in` (B == 1: the identity).  fill_value, mean, stdv: device f32 [3], all three always given.
 * Refused, nothing launched: a null in, out, fill_value, mean, stdv, rects or donor (DSNT_ERR_ARG); B outside 1..65535,
 * S outside 1..4096, K outside 1..DSNT_OCCLUDE_MAX_RECTS, J outside 0..DSNT_OCCLUDE_MAX_JOINTS, not 1 <= side_min <=
 * side_max <= S (DSNT_ERR_SHAPE); an unknown fill or centre, p24 > 2^24, J > 0 without coords or occluded, joint centring
 * of J > 0 joints without mask, in and out overlapping (DSNT_ERR_ARG).  S % 4 == 0 with 16-byte aligned tensors moves 16
 * bytes per access, anything else single floats.  Bit-reproducible (no atomics). */
#define DSNT_OCCLUDE_DOMAIN 0x4F43434Cu
#define DSNT_OCCLUDE_MAX_RECTS 8
#define DSNT_OCCLUDE_MAX_JOINTS 256
#define DSNT_OCCLUDE_FILL_VALUE 0
#define DSNT_OCCLUDE_FILL_NOISE 1
#define DSNT_OCCLUDE_FILL_PASTE 2
#define DSNT_OCCLUDE_CENTRE_UNIFORM 0
#define DSNT_OCCLUDE_CENTRE_JOINT 1
int dsnt_occlude(const float* in, float* out, int B, int S, int K, int side_min, int side_max, uint32_t p24, int fill,
                 int centre, const float* fill_value, const float* mean, const float* stdv, const float* coords,
                 const float* mask, int J, int32_t* rects, int32_t* donor, uint8_t* occluded, int draw, uint64_t seed,
                 uint64_t step, uint32_t draw_offset, void* stream);
/* Person crops of full images (dsnt.data.ImagePool.crop).  dsnt_version() >= 119.  pool: N RGB images, uint8 HWC, image i
 * at byte offset[i] (int64 [N]) with hw[i] = (h, w) (int32 [N][2]), pool_bytes the size of the buffer.  Sample b < B crops
 * image idx[b] (int64 [B]) with matrix[b] (f64 [B][3][3], image pixels -> [-1, 1]^2 crop coordinates) into out uint8
 * [B][R][R][3], equal bit for bit to Pillow's Image.transform((R, R), AFFINE, (a..f), BILINEAR) with the coefficients of
 * csrc/augment.hip; valid uint8 [B] = 1.  An index outside [0, N), an image record outside the pool or with a side outside
 * [1, 16384], or a matrix whose determinant is 0 or not finite reads nothing: zero crop, valid 0.  R <= 8192, B <= 65535.
 * Bit-reproducible (no atomics). */
int dsnt_crop_affine(const uint8_t* pool, int64_t pool_bytes, const int64_t* offset, const int32_t* hw, int64_t N,
                     const int64_t* idx, const double* matrix, int B, int R, uint8_t* out, uint8_t* valid, void* stream);
/* data.py:38-56 (ImageSpecs.convert) on a float image: x f32 [N][C][H][W] -> out f32 [N][C][S][S] =
 * (adaptive_avg_pool2d(x, S) - mean[c]) / stdv[c]; mean, stdv [C] (device). */
int dsnt_pool_normalize(const float* x, int N, int C, int H, int W, int S, const float* mean, const float* stdv,
                        float* out, void* stream);

/* ------------------------------------------------------------------ looking at predictions
 * train.py:455-483 (unconvert + util.draw_skeleton per image, the wrist heat-maps as pictures) for a whole batch in one
 * launch (dsnt.vis.render_pose; formulas in DESIGN.md section 15).  out uint8 [B][H][W][3] =
 * trunc(clamp(skeleton(heat(canvas)), 0, 255)); every byte is written once, out may be the uint8 canvas itself.
 * canvas, by canvas_kind: DSNT_RENDER_CANVAS_BLACK (canvas ignored); DSNT_RENDER_CANVAS_F32, model input f32 [B][3][H][W],
 * base = clamp((x * stdv[c] + mean[c]) * 255, 0, 255), each step rounded to fp32 (mean, stdv: HOST float[3], NULL = 0 and
 * 1); DSNT_RENDER_CANVAS_U8, uint8 [B][H][W][3].
 * Heat-map layer, when heatmaps != NULL: heatmaps f32 [B][J][h][w]; the peak of map (b, j) is peak[(b * J + j) *
 * peak_stride] (peak_stride 7 reads the stats buffer of dsnt_heatmap_stats in place); heat_rgb HOST float [J][3] in
 * [0, 1].  For every joint whose colour is not black v_j = clamp(sample_j / peak_j, 0, 1), 0 where peak_j is not positive
 * and finite or the sample is NaN; sample_j is bilinear with pixel centres aligned and the edge clamped, the stored value
 * when (h, w) == (H, W).  value_c = base_c + (255 - base_c) * (heat_alpha * clamp(sum_j v_j heat_rgb[j][c], 0, 1)).
 * Skeleton layer, when nbones > 0: coords f32 [B][J][2], normalised (u = (x + 1) W / 2, v = (y + 1) H / 2) or, with
 * pixel_coords != 0, continuous pixels (pixel i spans [i, i + 1)); mask f32 [B][J] or NULL; bone k joins joints
 * bone_joints[2k], bone_joints[2k + 1] (HOST int32) in colour bone_rgb[3k..] (HOST float, 0..255).  In table order, for
 * every bone with two finite ends: cov = clamp(width / 2 + 0.5 - d, 0, 1), d the distance of the pixel centre to the
 * segment, value = value (1 - cov) + rgb cov, rgb = (100, 100, 100) when mask is 0 at either end.  Then, when
 * joint_radius > 0, in joint order a disc cov = clamp(joint_radius + 0.5 - d, 0, 1) on every finite joint that a bone
 * names, in the colour of the first such bone, grey when masked.
 * All host tables travel as kernel arguments: no copy, no synchronisation.  DSNT_ERR_ARG: out, a used canvas, peak or
 * heat_rgb of a heat-map layer, coords or the bone table of a skeleton layer is NULL.  DSNT_ERR_SHAPE: unknown
 * canvas_kind; B outside 1..65535; H, W (h, w, peak_stride with heat-maps) outside 1..DSNT_RENDER_MAX_SIDE; with a layer,
 * J outside 1..DSNT_RENDER_MAX_JOINTS; nbones outside 0..DSNT_RENDER_MAX_BONES; a bone index outside 0..J-1; width not
 * positive.  Bit-reproducible (no atomics).  dsnt_version() >= 123. */
#define DSNT_RENDER_CANVAS_BLACK 0
#define DSNT_RENDER_CANVAS_F32 1
#define DSNT_RENDER_CANVAS_U8 2
#define DSNT_RENDER_MAX_JOINTS 64
#define DSNT_RENDER_MAX_BONES 32
#define DSNT_RENDER_MAX_SIDE 16384
int dsnt_render_pose(const void* canvas, int canvas_kind, const float* mean, const float* stdv, int B, int H, int W, int J,
                     const float* heatmaps, int h, int w, const float* peak, int64_t peak_stride, const float* heat_rgb,
                     float heat_alpha, const float* coords, const float* mask, int pixel_coords,
                     const int32_t* bone_joints, const float* bone_rgb, int nbones, float width, float joint_radius,
                     uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
