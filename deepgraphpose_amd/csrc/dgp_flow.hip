// gfx950 (MI355X / CDNA4): Farneback two-frame polynomial-expansion optical flow, parameterised like OpenCV's
// calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags = 0).  It replaces the
// host flow of learn_wt (DGP/models/fitdgp_util.py:454-467, called from fitdgp.py:771-775) that feeds the temporal clique.
//
// Kernels (every launch covers all frames or all pairs of the call through grid z):
//   flow_gray          uint8 BGR -> fp32 gray, OpenCV's fixed-point COLOR_BGR2GRAY (exact)                  once
//   flow_blur_resize   separable Gaussian of the FULL-RESOLUTION gray (REFLECT_101) sampled bilinearly at the level grid   per level
//   flow_polyexp       polynomial expansion, 5 coefficient planes per frame (LDS tile: vertical then horizontal pass)       per level
//   flow_init          flow of the coarser level upsampled x 1/pyr_scale (zero at the coarsest level) + the first M        per level
//   flow_iter          box mean of M (LDS tile with a winsize/2 halo) + 2x2 solve + M of the new flow (Jacobi)  `iterations` per level
// so 1 + levels_used * (3 + iterations) launches in all (25 with the reference's parameters).  fp32 arithmetic, no atomics: the
// result is a function of the inputs only.  The polynomial expansion depends on one frame, so it runs once per frame and level and
// frame t serves as "next" of pair t-1 and "prev" of pair t.
//
// Four details are written from knowledge of OpenCV's source and have not been checked against cv2 itself (to confirm once someone
// has it): (1) level 0 blurs with the fixed [0.25, 0.5, 0.25] (GaussianBlur with sigma 0 and ksize 3); (2) the box filter of the flow
// pass is the MEAN over winsize x winsize (visible only through the 1e-3 added to the determinant); (3) the border attenuation table
// {0.14, 0.14, 0.4472, 0.4472, 0.4472} over the 5 pixels next to each edge; (4) level sizes round half to even (cvRound).
#include "dgp_engine.h"

#include <cmath>
#include <string>
#include <vector>

namespace dgp {

constexpr int FLOW_TW = 64;            // output tile width of the LDS kernels (one wave per row segment)
constexpr int FLOW_TH = 16;            // output tile height (256 threads x 4 rows each)
constexpr int FLOW_MAX_R = 15;         // winsize <= 31
constexpr int FLOW_KMAX = 1024;        // longest level blur the LDS tap table holds
constexpr int FLOW_MIN_SIZE = 32;      // a level narrower or lower than this is not built (OpenCV's min_size)

struct PolyCoef {
    float g[8], xg[8], xxg[8];             // taps k = 0..poly_n (poly_n <= 7)
    float ig11, ig03, ig33, ig55;
};

__device__ __forceinline__ int refl101(int i, int n) {
    while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// (dst + 0.5) * ratio - 0.5 -> (floor clamped to [0, size-1], fraction; 0 where clamped)
__device__ __forceinline__ void lin_map(int d, float ratio, int size, int* i0, float* f) {
    const float s = ((float)d + 0.5f) * ratio - 0.5f;
    int i = (int)floorf(s);
    float fr = s - (float)i;
    if (i < 0) { i = 0; fr = 0.f; }
    if (i >= size - 1) { i = size - 1; fr = 0.f; }
    *i0 = i;
    *f = fr;
}

// ---- gray: gray = (1868 B + 9617 G + 4899 R + 8192) >> 14, channel 0 = B
__global__ __launch_bounds__(256) void flow_gray_kernel(const uint8_t* __restrict__ frames, long long n_pix, float* __restrict__ gray) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += (long long)gridDim.x * blockDim.x) {
        const uint8_t* p = frames + i * 3;
        const int v = (1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14;
        gray[i] = (float)v;
    }
}

// ---- level image: Gaussian blur (ksize, sigma; sigma == 0: [0.25, 0.5, 0.25]) of the full-resolution gray, REFLECT_101 borders, row
// filter before column filter, then bilinear resize to w x h.  A thread owns one output pixel: the rows sy0 - r .. sy0 + 1 + r and the
// columns sx0 - r .. sx0 + 1 + r of the source are each read once; a zero fraction skips the second column / row.
__global__ __launch_bounds__(256) void flow_blur_resize_kernel(const float* __restrict__ gray, int H, int W, float* __restrict__ img,
                                                               int h, int w, int ksize, double sigma, float rx, float ry) {
    __shared__ float taps[FLOW_KMAX];
    __shared__ double td[FLOW_KMAX];
    __shared__ double tsum;
    if (sigma <= 0.0) {
        if (threadIdx.x < 3) taps[threadIdx.x] = threadIdx.x == 1 ? 0.5f : 0.25f;
    } else {
        for (int i = threadIdx.x; i < ksize; i += blockDim.x) {
            const double x = i - (ksize - 1) * 0.5;
            td[i] = exp(-(x * x) / (2.0 * sigma * sigma));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int i = 0; i < ksize; ++i) s += td[i];
            tsum = 1.0 / s;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ksize; i += blockDim.x) taps[i] = (float)(td[i] * tsum);
    }
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float* src = gray + (long long)blockIdx.z * H * W;
    const int r = ksize / 2;
    int sx0, sy0;
    float fx, fy;
    lin_map(x, rx, W, &sx0, &fx);
    lin_map(y, ry, H, &sy0, &fy);
    const int ncol = fx != 0.f ? 2 * r + 2 : 2 * r + 1;
    const int nrow = fy != 0.f ? 2 * r + 2 : 2 * r + 1;
    float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
    for (int t = 0; t < nrow; ++t) {
        const float* row = src + (long long)refl101(sy0 - r + t, H) * W;
        float h0 = 0.f, h1 = 0.f;
        for (int i = 0; i < ncol; ++i) {
            const float v = row[refl101(sx0 - r + i, W)];
            if (i <= 2 * r) h0 += taps[i] * v;
            if (i >= 1) h1 += taps[i - 1] * v;
        }
        if (t <= 2 * r) { v00 += taps[t] * h0; v01 += taps[t] * h1; }
        if (t >= 1) { v10 += taps[t - 1] * h0; v11 += taps[t - 1] * h1; }
    }
    float out = v00;
    if (fx != 0.f) out = v00 * (1.f - fx) + v01 * fx;
    if (fy != 0.f) {
        const float b = fx != 0.f ? v10 * (1.f - fx) + v11 * fx : v10;
        out = out * (1.f - fy) + b * fy;
    }
    img[(long long)blockIdx.z * h * w + (long long)y * w + x] = out;
}

// ---- polynomial expansion of one level image: R planes [5][h][w] = (y, x, y^2, x^2, xy coefficients).  Vertical pass with rows
// clamped, horizontal pass with columns replicated (clamping the columns of the input tile replicates the vertical sums).
template <int n>
__global__ __launch_bounds__(256) void flow_polyexp_kernel(const float* __restrict__ img, int h, int w, float* __restrict__ R, PolyCoef c) {
    constexpr int TWX = FLOW_TW + 2 * n;
    __shared__ float tin[FLOW_TH + 2 * n][TWX];
    __shared__ float ts[3][FLOW_TH][TWX];
    constexpr int tw = FLOW_TW + 2 * n, th = FLOW_TH + 2 * n;
    const int x0 = blockIdx.x * FLOW_TW, y0 = blockIdx.y * FLOW_TH;
    const float* src = img + (long long)blockIdx.z * h * w;
    for (int i = threadIdx.x; i < tw * th; i += 256) {
        const int ly = i / tw, lx = i - ly * tw;
        const int gy = min(max(y0 - n + ly, 0), h - 1), gx = min(max(x0 - n + lx, 0), w - 1);
        tin[ly][lx] = src[(long long)gy * w + gx];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < tw * FLOW_TH; i += 256) {
        const int ly = i / tw, lx = i - ly * tw;
        const int cy = ly + n;
        float s0 = tin[cy][lx] * c.g[0], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 1; k <= n; ++k) {
            const float a = tin[cy - k][lx], b = tin[cy + k][lx];
            const float p = a + b;
            s0 += c.g[k] * p;
            s1 += c.xg[k] * (b - a);
            s2 += c.xxg[k] * p;
        }
        ts[0][ly][lx] = s0; ts[1][ly][lx] = s1; ts[2][ly][lx] = s2;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
    if (x >= w) return;
    const long long plane = (long long)h * w;
    float* dst = R + (long long)blockIdx.z * 5 * plane;
    for (int ly = threadIdx.x >> 6; ly < FLOW_TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= h) break;
        const int cx = lx + n;
        float b1 = ts[0][ly][cx] * c.g[0], b2 = 0.f, b3 = ts[1][ly][cx] * c.g[0], b4 = 0.f, b5 = ts[2][ly][cx] * c.g[0], b6 = 0.f;
#pragma unroll
        for (int k = 1; k <= n; ++k) {
            const float tg = ts[0][ly][cx + k] + ts[0][ly][cx - k];
            b1 += tg * c.g[k];
            b4 += tg * c.xxg[k];
            b2 += (ts[0][ly][cx + k] - ts[0][ly][cx - k]) * c.xg[k];
            b3 += (ts[1][ly][cx + k] + ts[1][ly][cx - k]) * c.g[k];
            b6 += (ts[1][ly][cx + k] - ts[1][ly][cx - k]) * c.xg[k];
            b5 += (ts[2][ly][cx + k] + ts[2][ly][cx - k]) * c.g[k];
        }
        const long long o = (long long)y * w + x;
        dst[o] = b3 * c.ig11;
        dst[plane + o] = b2 * c.ig11;
        dst[2 * plane + o] = b1 * c.ig03 + b5 * c.ig33;
        dst[3 * plane + o] = b1 * c.ig03 + b4 * c.ig33;
        dst[4 * plane + o] = b6 * c.ig55;
    }
}

// M of pixel (x, y) of a pair for the flow (dx, dy): R0 / R1 are the pair's coefficient planes [5][h][w], M planes [5][h][w]
__device__ __forceinline__ void flow_update_m(const float* __restrict__ R0, const float* __restrict__ R1, long long plane, int x, int y,
                                              int w, int h, float dx, float dy, float* __restrict__ M) {
    const long long o = (long long)y * w + x;
    float fx = (float)x + dx, fy = (float)y + dy;
    const float x1f = floorf(fx), y1f = floorf(fy);
    float r2, r3, r4, r5, r6;
    if (x1f >= 0.f && x1f < (float)(w - 1) && y1f >= 0.f && y1f < (float)(h - 1)) {
        const int x1 = (int)x1f, y1 = (int)y1f;
        fx -= x1f; fy -= y1f;
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        const long long q = (long long)y1 * w + x1;
        float v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float* p = R1 + k * plane + q;
            v[k] = a00 * p[0] + a01 * p[1] + a10 * p[w] + a11 * p[w + 1];
        }
        r2 = v[0]; r3 = v[1];
        r4 = (R0[2 * plane + o] + v[2]) * 0.5f;
        r5 = (R0[3 * plane + o] + v[3]) * 0.5f;
        r6 = (R0[4 * plane + o] + v[4]) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = R0[2 * plane + o];
        r5 = R0[3 * plane + o];
        r6 = R0[4 * plane + o] * 0.5f;
    }
    r2 = (R0[o] - r2) * 0.5f;
    r3 = (R0[plane + o] - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    if (x < 5 || x >= w - 5 || y < 5 || y >= h - 5) {
        // border[d] = {0.14, 0.14, 0.4472, 0.4472, 0.4472}[d] at distance d < 5 from an edge
        auto border = [](int d) { return d < 5 ? (d < 2 ? 0.14f : 0.4472f) : 1.f; };
        const float s = border(x) * border(w - x - 1) * border(y) * border(h - y - 1);
        r2 *= s; r3 *= s; r4 *= s; r5 *= s; r6 *= s;
    }
    M[o] = r4 * r4 + r6 * r6;
    M[plane + o] = (r4 + r5) * r6;
    M[2 * plane + o] = r5 * r5 + r6 * r6;
    M[3 * plane + o] = r4 * r2 + r6 * r3;
    M[4 * plane + o] = r6 * r2 + r5 * r3;
}

// ---- first M of a level: flow = 0 (coarsest level) or the coarser level's flow resized bilinearly and multiplied by 1 / pyr_scale
__global__ __launch_bounds__(256) void flow_init_kernel(const float* __restrict__ R, const float2* __restrict__ prev, int pw, int ph,
                                                        float rx, float ry, float up, float2* __restrict__ flow, float* __restrict__ M,
                                                        int w, int h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int p = blockIdx.z;
    const long long plane = (long long)h * w;
    float2 f = make_float2(0.f, 0.f);
    if (prev) {
        int sx, sy;
        float fx, fy;
        lin_map(x, rx, pw, &sx, &fx);
        lin_map(y, ry, ph, &sy, &fy);
        const float2* s = prev + (long long)p * ph * pw;
        const int sx1 = min(sx + 1, pw - 1), sy1 = min(sy + 1, ph - 1);
        const float2 a = s[(long long)sy * pw + sx], b = s[(long long)sy * pw + sx1];
        const float2 c = s[(long long)sy1 * pw + sx], d = s[(long long)sy1 * pw + sx1];
        const float t0x = a.x * (1.f - fx) + b.x * fx, t0y = a.y * (1.f - fx) + b.y * fx;
        const float t1x = c.x * (1.f - fx) + d.x * fx, t1y = c.y * (1.f - fx) + d.y * fx;
        f.x = (t0x * (1.f - fy) + t1x * fy) * up;
        f.y = (t0y * (1.f - fy) + t1y * fy) * up;
    }
    flow[(long long)p * plane + (long long)y * w + x] = f;
    flow_update_m(R + (long long)p * 5 * plane, R + (long long)(p + 1) * 5 * plane, plane, x, y, w, h, f.x, f.y,
                  M + (long long)p * 5 * plane);
}

// ---- one flow pass: winsize x winsize box mean of the 5 M planes (replicated borders; LDS tile with an r-pixel halo, vertical then
// horizontal sums, one plane at a time), 2x2 solve, and -- unless this is the level's last pass -- M of the new flow into M_out.
// out_mag (nullable): |dx| + |dy|, written on the last pass of level 0.
__global__ __launch_bounds__(256) void flow_iter_kernel(const float* __restrict__ M_in, const float* __restrict__ R, int w, int h, int r,
                                                        float inv_area, float* __restrict__ M_out, float2* __restrict__ flow,
                                                        float* __restrict__ out_mag) {
    constexpr int TWX = FLOW_TW + 2 * FLOW_MAX_R;
    __shared__ float tin[FLOW_TH + 2 * FLOW_MAX_R][TWX];
    __shared__ float tv[FLOW_TH][TWX];
    const int tw = FLOW_TW + 2 * r, th = FLOW_TH + 2 * r;
    const int x0 = blockIdx.x * FLOW_TW, y0 = blockIdx.y * FLOW_TH;
    const int p = blockIdx.z;
    const long long plane = (long long)h * w;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    float acc[5][FLOW_TH / 4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float* src = M_in + ((long long)p * 5 + k) * plane;
        for (int i = threadIdx.x; i < tw * th; i += 256) {
            const int ty = i / tw, tx = i - ty * tw;
            const int gy = min(max(y0 - r + ty, 0), h - 1), gx = min(max(x0 - r + tx, 0), w - 1);
            tin[ty][tx] = src[(long long)gy * w + gx];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < tw * FLOW_TH; i += 256) {
            const int ty = i / tw, tx = i - ty * tw;
            float s = 0.f;
            for (int j = 0; j <= 2 * r; ++j) s += tin[ty + j][tx];
            tv[ty][tx] = s;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < FLOW_TH / 4; ++q) {
            const int ty = ly0 + 4 * q;
            float s = 0.f;
            for (int j = 0; j <= 2 * r; ++j) s += tv[ty][lx + j];
            acc[k][q] = s;
        }
        __syncthreads();
    }
    const int x = x0 + lx;
    if (x >= w) return;
    const float* R0 = R + (long long)p * 5 * plane;
    const float* R1 = R0 + 5 * plane;
#pragma unroll
    for (int q = 0; q < FLOW_TH / 4; ++q) {
        const int y = y0 + ly0 + 4 * q;
        if (y >= h) break;
        const float g11 = acc[0][q] * inv_area, g12 = acc[1][q] * inv_area, g22 = acc[2][q] * inv_area;
        const float h1 = acc[3][q] * inv_area, h2 = acc[4][q] * inv_area;
        const float idet = 1.f / (g11 * g22 - g12 * g12 + 1e-3f);
        const float dx = (g11 * h2 - g12 * h1) * idet;
        const float dy = (g22 * h1 - g12 * h2) * idet;
        const long long o = (long long)p * plane + (long long)y * w + x;
        flow[o] = make_float2(dx, dy);
        if (out_mag) out_mag[o] = fabsf(dx) + fabsf(dy);
        if (M_out) flow_update_m(R0, R1, plane, x, y, w, h, dx, dy, M_out + (long long)p * 5 * plane);
    }
}

struct FlowLevel {
    int w, h, ksize;
    double sigma;
};

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// validation + level plan (OpenCV's: the pyramid stops before the first level narrower or lower than 32 pixels)
static int flow_plan(int32_t n_frames, int32_t H, int32_t W, const dgp_flow_params* p, std::vector<FlowLevel>* lv, size_t* bytes) {
    if (!p) return fail(DGP_ERR_INVALID, "optical flow: null parameters");
    if (!(p->pyr_scale > 0.0 && p->pyr_scale < 1.0)) return fail(DGP_ERR_INVALID, "optical flow: pyr_scale must be in (0, 1)");
    if (p->levels < 0) return fail(DGP_ERR_INVALID, "optical flow: levels must be >= 0");
    if (p->winsize < 3 || p->winsize > 2 * FLOW_MAX_R + 1 || (p->winsize & 1) == 0)
        return fail(DGP_ERR_INVALID, "optical flow: winsize must be odd, 3..31");
    if (p->iterations < 1) return fail(DGP_ERR_INVALID, "optical flow: iterations must be >= 1");
    if (p->poly_n != 5 && p->poly_n != 7) return fail(DGP_ERR_INVALID, "optical flow: poly_n must be 5 or 7");
    if (!(p->poly_sigma > 0.0)) return fail(DGP_ERR_INVALID, "optical flow: poly_sigma must be > 0");
    if (p->flags != 0) return fail(DGP_ERR_INVALID, "optical flow: flags must be 0 (Gaussian window / initial flow are not built)");
    if (H < 16 || W < 16) return fail(DGP_ERR_INVALID, "optical flow: frames must be at least 16 x 16");
    if (n_frames < 2) return fail(DGP_ERR_INVALID, "optical flow: needs at least 2 frames");
    int levels = 0;
    double s = 1.0;
    for (; levels < p->levels; ++levels) {
        s *= p->pyr_scale;
        if (W * s < FLOW_MIN_SIZE || H * s < FLOW_MIN_SIZE) break;
    }
    lv->clear();
    for (int k = 0; k <= levels; ++k) {
        double scale = 1.0;
        for (int i = 0; i < k; ++i) scale *= p->pyr_scale;
        FlowLevel L;
        L.sigma = (1.0 / scale - 1.0) * 0.5;
        L.ksize = std::max((int)std::lrint(L.sigma * 5.0) | 1, 3);
        L.w = (int)std::lrint(W * scale);
        L.h = (int)std::lrint(H * scale);
        if (L.ksize >= FLOW_KMAX) return fail(DGP_ERR_INVALID, "optical flow: level blur longer than 1023 taps (frame too large for the plan)");
        lv->push_back(L);
    }
    const size_t T = (size_t)n_frames, P = T - 1, px = (size_t)H * W;
    *bytes = 2 * align256(T * px * 4) + align256(T * 5 * px * 4) + 2 * align256(P * px * 8) + 2 * align256(P * 5 * px * 4);
    return DGP_OK;
}

// Gaussian of the polynomial expansion and the entries of the inverse moment matrix it needs (basis 1, x, y, x^2, y^2, xy)
static PolyCoef poly_coef(int n, double sigma) {
    PolyCoef c{};
    std::vector<float> g(2 * n + 1);
    double s = 0.0;
    for (int x = -n; x <= n; ++x) {
        g[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma));
        s += g[x + n];
    }
    s = 1.0 / s;
    for (int x = -n; x <= n; ++x) g[x + n] = (float)(g[x + n] * s);
    for (int k = 0; k <= n; ++k) {
        c.g[k] = g[k + n];
        c.xg[k] = (float)(k * g[k + n]);
        c.xxg[k] = (float)(k * k * g[k + n]);
    }
    double G[6][6] = {};
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const double gg = (double)g[y + n] * g[x + n];
            G[0][0] += gg;
            G[1][1] += gg * x * x;
            G[3][3] += gg * x * x * x * x;
            G[5][5] += gg * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    // Gauss-Jordan inverse with partial pivoting (G is symmetric positive definite)
    double A[6][12] = {};
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) A[i][j] = G[i][j];
        A[i][6 + i] = 1.0;
    }
    for (int col = 0; col < 6; ++col) {
        int piv = col;
        for (int i = col + 1; i < 6; ++i)
            if (std::fabs(A[i][col]) > std::fabs(A[piv][col])) piv = i;
        if (piv != col)
            for (int j = 0; j < 12; ++j) std::swap(A[col][j], A[piv][j]);
        const double d = 1.0 / A[col][col];
        for (int j = 0; j < 12; ++j) A[col][j] *= d;
        for (int i = 0; i < 6; ++i) {
            if (i == col) continue;
            const double f = A[i][col];
            for (int j = 0; j < 12; ++j) A[i][j] -= f * A[col][j];
        }
    }
    c.ig11 = (float)A[1][6 + 1];
    c.ig03 = (float)A[0][6 + 3];
    c.ig33 = (float)A[3][6 + 3];
    c.ig55 = (float)A[5][6 + 5];
    return c;
}

static dim3 tiles(int w, int h, int tw, int th, int z) { return dim3((unsigned)((w + tw - 1) / tw), (unsigned)((h + th - 1) / th), (unsigned)z); }

}  // namespace dgp

using namespace dgp;

extern "C" {

int dgp_optical_flow_scratch_bytes(int32_t n_frames, int32_t H, int32_t W, const dgp_flow_params* p, size_t* bytes, int32_t* levels_used) {
    std::vector<FlowLevel> lv;
    size_t b = 0;
    const int rc = flow_plan(n_frames, H, W, p, &lv, &b);
    if (rc != DGP_OK) return rc;
    if (bytes) *bytes = b;
    if (levels_used) *levels_used = (int32_t)lv.size() - 1;
    return DGP_OK;
}

int dgp_optical_flow(const uint8_t* frames, int32_t n_frames, int32_t H, int32_t W, const dgp_flow_params* p, float* flow,
                     float* magnitude, void* scratch, size_t scratch_bytes, void* stream) {
    std::vector<FlowLevel> lv;
    size_t need = 0;
    const int rc = flow_plan(n_frames, H, W, p, &lv, &need);
    if (rc != DGP_OK) return rc;
    if (!frames || !scratch) return fail(DGP_ERR_INVALID, "dgp_optical_flow: null frames or scratch");
    if (!flow && !magnitude) return fail(DGP_ERR_INVALID, "dgp_optical_flow: neither flow nor magnitude requested");
    if (scratch_bytes < need) return fail(DGP_ERR_INVALID, "dgp_optical_flow: scratch too small");
    const hipStream_t s = (hipStream_t)stream;
    const int T = n_frames, P = n_frames - 1;
    const size_t px = (size_t)H * W;
    char* sc = (char*)scratch;
    float* gray = (float*)sc;              sc += align256((size_t)T * px * 4);
    float* img = (float*)sc;               sc += align256((size_t)T * px * 4);
    float* R = (float*)sc;                 sc += align256((size_t)T * 5 * px * 4);
    float2* fl[2] = {(float2*)sc, nullptr}; sc += align256((size_t)P * px * 8);
    fl[1] = (float2*)sc;                   sc += align256((size_t)P * px * 8);
    float* Mb[2] = {(float*)sc, nullptr};  sc += align256((size_t)P * 5 * px * 4);
    Mb[1] = (float*)sc;
    const PolyCoef pc = poly_coef(p->poly_n, p->poly_sigma);
    const long long npx = (long long)T * px;
    hipLaunchKernelGGL(flow_gray_kernel, dim3((unsigned)std::min<long long>((npx + 255) / 256, 8192)), dim3(256), 0, s, frames, npx, gray);
    const int r = p->winsize / 2;
    const float inv_area = (float)(1.0 / ((double)p->winsize * p->winsize));
    const float up = (float)(1.0 / p->pyr_scale);
    int cur = 0;
    const float2* prev = nullptr;
    int pw = 0, ph = 0;
    for (int k = (int)lv.size() - 1; k >= 0; --k) {
        const FlowLevel& L = lv[k];
        hipLaunchKernelGGL(flow_blur_resize_kernel, tiles(L.w, L.h, 64, 4, T), dim3(256), 0, s, gray, H, W, img, L.h, L.w, L.ksize,
                           k == 0 ? 0.0 : L.sigma, (float)((double)W / L.w), (float)((double)H / L.h));
        if (p->poly_n == 5) hipLaunchKernelGGL(flow_polyexp_kernel<5>, tiles(L.w, L.h, FLOW_TW, FLOW_TH, T), dim3(256), 0, s, img, L.h, L.w, R, pc);
        else hipLaunchKernelGGL(flow_polyexp_kernel<7>, tiles(L.w, L.h, FLOW_TW, FLOW_TH, T), dim3(256), 0, s, img, L.h, L.w, R, pc);
        float2* f = fl[cur];
        hipLaunchKernelGGL(flow_init_kernel, tiles(L.w, L.h, 64, 4, P), dim3(256), 0, s, R, prev, pw, ph,
                           prev ? (float)((double)pw / L.w) : 1.f, prev ? (float)((double)ph / L.h) : 1.f, up, f, Mb[0], L.w, L.h);
        for (int it = 0; it < p->iterations; ++it) {
            const bool last = it == p->iterations - 1;
            float2* dst = (last && k == 0 && flow) ? (float2*)flow : f;
            hipLaunchKernelGGL(flow_iter_kernel, tiles(L.w, L.h, FLOW_TW, FLOW_TH, P), dim3(256), 0, s, Mb[it & 1], R, L.w, L.h, r,
                               inv_area, last ? nullptr : Mb[(it + 1) & 1], dst, (last && k == 0) ? magnitude : nullptr);
        }
        prev = f;
        pw = L.w;
        ph = L.h;
        cur ^= 1;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("optical flow: ") + hipGetErrorString(e));
    return DGP_OK;
}

}  // extern "C"
