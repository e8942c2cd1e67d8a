// The per-op kernels behind dsnt.nn, each pair followed by its entry points: heat-map normalisation, coordinate
// expectation, Gaussian targets, Euclidean loss, masked average and the `fc` output strategy.  Rows: head_row.h.
#include "head_row.h"

// ------------------------------------------------------------------ preact (model.py:24-45)
template <int VEC, bool CACHED>
__global__ __launch_bounds__(HB) void preact_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         int hw, int mode, float thr, float eps) {
    __shared__ float red[16];
    const size_t off = (size_t)blockIdx.x * hw;
    Row<VEC, CACHED> row;
    row.load(x + off, hw);
    float* out = y + off;
    preact_row(row, mode, thr, eps, red, [&](int i, float p) { out[i] = p; });
}

template <int VEC, bool CACHED>
__global__ __launch_bounds__(HB) void preact_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ gy, float* __restrict__ gx,
                                                         int hw, int mode, float eps) {
    __shared__ float red[16];
    const size_t off = (size_t)blockIdx.x * hw;
    Row<VEC, CACHED> py;
    py.load(y + off, hw);
    const float* g = gy + off;
    float* out = gx + off;
    if (mode <= 1) {
        float s[1] = {0.f};
        py.each([&](int i, float p) { s[0] = fmaf(p, g[i], s[0]); });
        block_sum<1>(s, red);
        py.each([&](int i, float p) { out[i] = p * (g[i] - s[0]); });
    } else {
        const float* xr = x + off;
        float s[2] = {0.f, 0.f};   // sum f(x), sum g*y
        py.each([&](int i, float p) { s[0] += preact_act(mode, xr[i]); s[1] = fmaf(p, g[i], s[1]); });
        block_sum<2>(s, red);
        const float inv = 1.f / (s[0] + eps);
        py.each([&](int i, float) {
            const float v = xr[i];
            float d;
            if (mode == 2) d = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
            else if (mode == 3) d = v > 0.f ? 1.f : 0.f;
            else { const float sg = 1.f / (1.f + expf(-v)); d = sg * (1.f - sg); }
            out[i] = d * (g[i] - s[1]) * inv;
        });
    }
}

extern "C" int dsnt_preact_fwd(const float* x, float* y, int64_t rows, int hw, int mode, float threshold,
                               float eps, void* stream) {
    DSNT_REQUIRE(x && y, DSNT_ERR_ARG, "dsnt_preact_fwd: null tensor");
    DSNT_REQUIRE(mode >= 0 && mode <= 4, DSNT_ERR_ARG, "dsnt_preact_fwd: unknown mode %d", mode);
    if (int e = check_rows("dsnt_preact_fwd", rows, 1, hw)) return e;
    ROW_DISPATCH(preact_fwd_kernel, (int)rows, hw, dsnt_aligned16(x), x, y, hw, mode, threshold, eps);
    DSNT_CHECK_LAUNCH("dsnt_preact_fwd");
}

extern "C" int dsnt_preact_bwd(const float* x, const float* y, const float* gy, float* gx, int64_t rows,
                               int hw, int mode, float threshold, float eps, void* stream) {
    (void)threshold;
    DSNT_REQUIRE(y && gy && gx && (mode <= 1 || x), DSNT_ERR_ARG, "dsnt_preact_bwd: null tensor");
    DSNT_REQUIRE(mode >= 0 && mode <= 4, DSNT_ERR_ARG, "dsnt_preact_bwd: unknown mode %d", mode);
    if (int e = check_rows("dsnt_preact_bwd", rows, 1, hw)) return e;
    ROW_DISPATCH(preact_bwd_kernel, (int)rows, hw, dsnt_aligned16(y), x, y, gy, gx, hw, mode, eps);
    DSNT_CHECK_LAUNCH("dsnt_preact_bwd");
}

// ------------------------------------------------------------------ dsnt (nn.py:25-78)
template <int VEC, bool CACHED>
__global__ __launch_bounds__(HB) void expect_fwd_kernel(const float* __restrict__ hm, float* __restrict__ coords,
                                                         int h, int w) {
    __shared__ float red[16];
    const int hw = h * w;
    Row<VEC, CACHED> row;
    row.load(hm + (size_t)blockIdx.x * hw, hw);
    const Grid2 g(h, w);
    float s[2] = {0.f, 0.f};
    row.each([&](int i, float p) {
        float x, y; g.xy(i, x, y);
        s[0] = fmaf(x, p, s[0]); s[1] = fmaf(y, p, s[1]);
    });
    block_sum<2>(s, red);
    if (threadIdx.x == 0) { coords[2 * (size_t)blockIdx.x] = s[0]; coords[2 * (size_t)blockIdx.x + 1] = s[1]; }
}

__global__ __launch_bounds__(HB) void expect_bwd_kernel(const float* __restrict__ gc, float* __restrict__ ghm,
                                                         int h, int w) {
    const int hw = h * w;
    const float gx = gc[2 * (size_t)blockIdx.x], gy = gc[2 * (size_t)blockIdx.x + 1];
    float* out = ghm + (size_t)blockIdx.x * hw;
    const Grid2 g(h, w);
    for (int i = threadIdx.x; i < hw; i += HB) {
        float x, y; g.xy(i, x, y);
        out[i] = gx * x + gy * y;
    }
}

extern "C" int dsnt_expect_fwd(const float* hm, float* coords, int64_t rows, int h, int w, void* stream) {
    DSNT_REQUIRE(hm && coords, DSNT_ERR_ARG, "dsnt_expect_fwd: null tensor");
    if (int e = check_rows("dsnt_expect_fwd", rows, h, w)) return e;
    ROW_DISPATCH(expect_fwd_kernel, (int)rows, h * w, dsnt_aligned16(hm), hm, coords, h, w);
    DSNT_CHECK_LAUNCH("dsnt_expect_fwd");
}

extern "C" int dsnt_expect_bwd(const float* gcoords, float* ghm, int64_t rows, int h, int w, void* stream) {
    DSNT_REQUIRE(gcoords && ghm, DSNT_ERR_ARG, "dsnt_expect_bwd: null tensor");
    if (int e = check_rows("dsnt_expect_bwd", rows, h, w)) return e;
    DSNT_LAUNCH(expect_bwd_kernel, dim3((int)rows), dim3(HB), 0, (hipStream_t)stream, gcoords, ghm, h, w);
    DSNT_CHECK_LAUNCH("dsnt_expect_bwd");
}

// ------------------------------------------------------------------ make_gauss (nn.py:168-205)
__global__ __launch_bounds__(HB) void make_gauss_kernel(const float* __restrict__ coords, float* __restrict__ out,
                                                         int h, int w, float k) {
    __shared__ float red[16];
    const int hw = h * w;
    const float mx = coords[2 * (size_t)blockIdx.x], my = coords[2 * (size_t)blockIdx.x + 1];
    float* o = out + (size_t)blockIdx.x * hw;
    const Grid2 g(h, w);
    float s[1] = {0.f};
    for (int i = threadIdx.x; i < hw; i += HB) {
        float x, y; g.xy(i, x, y);
        s[0] += gauss_e(x, y, mx, my, k);
    }
    block_sum<1>(s, red);
    const float z = s[0] + 1e-24f;
    for (int i = threadIdx.x; i < hw; i += HB) {
        float x, y; g.xy(i, x, y);
        o[i] = gauss_e(x, y, mx, my, k) / z;
    }
}

// d/d(mu) of the above (the reference's make_gauss is differentiable in `coords`, nn.py:180-203):
//   g_i = e_i / Z,  d g_i / d mu_x = g_i ((x_i - mu_x) - sum_j g_j (x_j - mu_x)) / sigma^2
//   dL/d mu_x = (sum_i G_i g_i (x_i - mu_x) - m_x sum_i G_i g_i) / sigma^2,  m_x = sum_j g_j (x_j - mu_x)
// The Gaussian is re-evaluated in registers (one pass for Z, one over the incoming gradient G): one HBM read.
__global__ __launch_bounds__(HB) void make_gauss_bwd_kernel(const float* __restrict__ coords, const float* __restrict__ gout,
                                                             float* __restrict__ gcoords, int h, int w, float k) {
    __shared__ float red[32];
    const int hw = h * w;
    const float mx = coords[2 * (size_t)blockIdx.x], my = coords[2 * (size_t)blockIdx.x + 1];
    const float* G = gout + (size_t)blockIdx.x * hw;
    const Grid2 g(h, w);
    float z[1] = {0.f};
    for (int i = threadIdx.x; i < hw; i += HB) {
        float x, y; g.xy(i, x, y);
        z[0] += gauss_e(x, y, mx, my, k);
    }
    block_sum<1>(z, red);
    const float inv = 1.f / (z[0] + 1e-24f);
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // sum G g, sum G g dx, sum G g dy, sum g dx, sum g dy
    for (int i = threadIdx.x; i < hw; i += HB) {
        float x, y; g.xy(i, x, y);
        const float dx = x - mx, dy = y - my;
        const float q = gauss_e(x, y, mx, my, k) * inv;
        const float gq = G[i] * q;
        s[0] += gq; s[1] = fmaf(gq, dx, s[1]); s[2] = fmaf(gq, dy, s[2]);
        s[3] = fmaf(q, dx, s[3]); s[4] = fmaf(q, dy, s[4]);
    }
    block_sum<5>(s, red);
    if (threadIdx.x == 0) {
        const float is2 = -2.f * k;            // 1 / sigma^2
        gcoords[2 * (size_t)blockIdx.x] = (s[1] - s[3] * s[0]) * is2;
        gcoords[2 * (size_t)blockIdx.x + 1] = (s[2] - s[4] * s[0]) * is2;
    }
}

extern "C" int dsnt_make_gauss(const float* coords, float* out, int64_t rows, int h, int w, float sigma, void* stream) {
    DSNT_REQUIRE(coords && out, DSNT_ERR_ARG, "dsnt_make_gauss: null tensor");
    DSNT_REQUIRE(sigma > 0.f, DSNT_ERR_ARG, "dsnt_make_gauss: sigma must be positive");
    if (int e = check_rows("dsnt_make_gauss", rows, h, w)) return e;
    DSNT_LAUNCH(make_gauss_kernel, dim3((int)rows), dim3(HB), 0, (hipStream_t)stream, coords, out, h, w, gauss_k(sigma));
    DSNT_CHECK_LAUNCH("dsnt_make_gauss");
}

extern "C" int dsnt_make_gauss_bwd(const float* coords, const float* g_out, float* g_coords, int64_t rows, int h, int w,
                                   float sigma, void* stream) {
    DSNT_REQUIRE(coords && g_out && g_coords, DSNT_ERR_ARG, "dsnt_make_gauss_bwd: null tensor");
    DSNT_REQUIRE(sigma > 0.f, DSNT_ERR_ARG, "dsnt_make_gauss_bwd: sigma must be positive");
    if (int e = check_rows("dsnt_make_gauss_bwd", rows, h, w)) return e;
    DSNT_LAUNCH(make_gauss_bwd_kernel, dim3((int)rows), dim3(HB), 0, (hipStream_t)stream, coords, g_out, g_coords, h, w,
                gauss_k(sigma));
    DSNT_CHECK_LAUNCH("dsnt_make_gauss_bwd");
}

// ------------------------------------------------------------------ euclid / masked average
__global__ void euclid_fwd_kernel(const float* __restrict__ a, const float* __restrict__ t, float* __restrict__ dist,
                                  long n, int d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int j = 0; j < d; ++j) { const float df = a[i * d + j] - t[i * d + j]; s += df * df; }
    dist[i] = sqrtf(s);
}
__global__ void euclid_bwd_kernel(const float* __restrict__ a, const float* __restrict__ t,
                                  const float* __restrict__ dist, const float* __restrict__ gd,
                                  float* __restrict__ ga, long n, int d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // d sqrt(s)/da = (a-t)/dist; at dist == 0 the reference's autograd gives 0 * inf = NaN
    const float f = gd[i] / (2.f * dist[i]);
    for (int j = 0; j < d; ++j) ga[i * d + j] = f * (2.f * (a[i * d + j] - t[i * d + j]));
}

extern "C" int dsnt_euclid_fwd(const float* actual, const float* target, float* dist, int64_t n, int d, void* stream) {
    DSNT_REQUIRE(actual && target && dist && n > 0 && d > 0, DSNT_ERR_ARG, "dsnt_euclid_fwd: bad argument");
    DSNT_LAUNCH(euclid_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       actual, target, dist, (long)n, d);
    DSNT_CHECK_LAUNCH("dsnt_euclid_fwd");
}

extern "C" int dsnt_euclid_bwd(const float* actual, const float* target, const float* dist, const float* g_dist,
                               float* g_actual, int64_t n, int d, void* stream) {
    DSNT_REQUIRE(actual && target && dist && g_dist && g_actual && n > 0 && d > 0, DSNT_ERR_ARG,
                 "dsnt_euclid_bwd: bad argument");
    DSNT_LAUNCH(euclid_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       actual, target, dist, g_dist, g_actual, (long)n, d);
    DSNT_CHECK_LAUNCH("dsnt_euclid_bwd");
}

__global__ __launch_bounds__(HB) void masked_avg_fwd_kernel(const float* __restrict__ l, const float* __restrict__ m,
                                                             float* __restrict__ out2, long n) {
    __shared__ float red[16];
    float s[2] = {0.f, 0.f};
    for (long i = threadIdx.x; i < n; i += HB) {
        const float w = m ? m[i] : 1.f;
        s[0] += m ? l[i] * w : l[i];
        s[1] += w;
    }
    block_sum<2>(s, red);
    if (threadIdx.x == 0) {
        const float denom = fmaxf(s[1], 1.f);
        out2[0] = s[0] / denom;
        out2[1] = denom;
    }
}
__global__ void masked_avg_bwd_kernel(const float* __restrict__ g, const float* __restrict__ m,
                                      const float* __restrict__ out2, float* __restrict__ gl, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gl[i] = g[0] * (m ? m[i] : 1.f) / out2[1];
}

extern "C" int dsnt_masked_avg_fwd(const float* losses, const float* mask, float* out2, int64_t n, void* stream) {
    DSNT_REQUIRE(losses && out2 && n > 0, DSNT_ERR_ARG, "dsnt_masked_avg_fwd: bad argument");
    DSNT_LAUNCH(masked_avg_fwd_kernel, dim3(1), dim3(HB), 0, (hipStream_t)stream, losses, mask, out2, (long)n);
    DSNT_CHECK_LAUNCH("dsnt_masked_avg_fwd");
}

extern "C" int dsnt_masked_avg_bwd(const float* g_out, const float* mask, const float* out2, float* g_losses,
                                   int64_t n, void* stream) {
    DSNT_REQUIRE(g_out && out2 && g_losses && n > 0, DSNT_ERR_ARG, "dsnt_masked_avg_bwd: bad argument");
    DSNT_LAUNCH(masked_avg_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       g_out, mask, out2, g_losses, (long)n);
    DSNT_CHECK_LAUNCH("dsnt_masked_avg_bwd");
}

// ---------------------------------------------------------------- 'fc' output strategy
// out[row][k] = sum_i hm[row][i] * W[k][i] + b[k], k = 0,1 — `out_fc = nn.Linear(H*W, 2)` applied to the flattened
// heat-maps (reference model.py:222-223, 293-303; :196-198 for ResNet).  One workgroup per row.
__global__ __launch_bounds__(256) void fc2_fwd_kernel(const float* __restrict__ hm, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ out, int hw) {
    __shared__ float red[2][4];
    const float* row = hm + (size_t)blockIdx.x * hw;
    float a0 = 0.f, a1 = 0.f;
    for (int i = threadIdx.x; i < hw; i += 256) {
        const float v = row[i];
        a0 = fmaf(v, w[i], a0);
        a1 = fmaf(v, w[hw + i], a1);
    }
    for (int o = 32; o >= 1; o >>= 1) { a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a0; red[1][threadIdx.x >> 6] = a1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        out[(size_t)blockIdx.x * 2 + threadIdx.x] = s + (b ? b[threadIdx.x] : 0.f);
    }
}

extern "C" int dsnt_fc2_fwd(const float* hm, const float* w, const float* b, float* out, int64_t rows, int hw,
                            void* stream) {
    DSNT_REQUIRE(hm && w && out && rows > 0 && rows < (1LL << 31) && hw > 0, DSNT_ERR_ARG, "dsnt_fc2_fwd: bad argument");
    DSNT_LAUNCH(fc2_fwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, hm, w, b, out, hw);
    DSNT_CHECK_LAUNCH("dsnt_fc2_fwd");
}

// ghm[row][i] = g[row][0] W[0][i] + g[row][1] W[1][i];  gW[k][i] = sum_row g[row][k] hm[row][i];  gb[k] = sum_row g[row][k].
// One thread per column i walks the rows in order (deterministic); rows = B * 16 is small.
__global__ __launch_bounds__(256) void fc2_bwd_kernel(const float* __restrict__ g, const float* __restrict__ hm,
                                                      const float* __restrict__ w, float* __restrict__ ghm,
                                                      float* __restrict__ gw, float* __restrict__ gb, int rows, int hw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < hw) {
        const float w0 = w[i], w1 = w[hw + i];
        float s0 = 0.f, s1 = 0.f;
        for (int r = 0; r < rows; ++r) {
            const float g0 = g[2 * r], g1 = g[2 * r + 1];
            const float v = hm[(size_t)r * hw + i];
            if (ghm) ghm[(size_t)r * hw + i] = fmaf(g0, w0, g1 * w1);
            s0 = fmaf(g0, v, s0);
            s1 = fmaf(g1, v, s1);
        }
        gw[i] = s0;
        gw[hw + i] = s1;
    }
    if (gb && blockIdx.x == 0 && threadIdx.x < 2) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += g[2 * r + threadIdx.x];
        gb[threadIdx.x] = s;
    }
}

extern "C" int dsnt_fc2_bwd(const float* g, const float* hm, const float* w, float* ghm, float* gw, float* gb,
                            int64_t rows, int hw, void* stream) {
    DSNT_REQUIRE(g && hm && w && gw && rows > 0 && rows < (1LL << 31) && hw > 0, DSNT_ERR_ARG, "dsnt_fc2_bwd: bad argument");
    DSNT_LAUNCH(fc2_bwd_kernel, dim3((hw + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, hm, w, ghm, gw, gb,
                       (int)rows, hw);
    DSNT_CHECK_LAUNCH("dsnt_fc2_bwd");
}
