// gfx950 (MI355X / CDNA4): the augmenters of the DGP drivers' labeled frames (build_aug / data_aug, DGP/models/fitdgp_util.py:412-451;
// host counterpart: deepgraphpose_amd/augment.py) applied on the device from a plan drawn on the host.  Every random number is drawn
// there, in the host pipeline's order; a kernel gets the drawn parameters and one frame.
//
// One frame per call, uint8 [H][W][3] packed, src != dst, on the caller's stream.  A thread owns one output pixel (three bytes): plain
// byte loads and stores, no LDS, no atomics.  At one or two 1.9 MB frames per batch every launch is latency bound, so nothing here is
// tuned for bandwidth.  All argument checks happen on the host in the C entries, before anything is launched.
//
//   affine   Pillow's Image.transform(AFFINE, BILINEAR) in double, truncated: the bytes are Pillow's.  fliplr is the same kernel.
//   blur3    the host's 3 x 3 fp32 sum in the host loop's order, edge-replicated, rintf.  The bytes are the host stage's.
//   dropout  nearest-neighbour upsampling of a coarse bool mask, integer index arithmetic.  The bytes are the host stage's.
//   elastic  out[p] = in[p + d(p)], d the align-corners bilinear upsampling (x 4) of a coarse fp32 field, bilinear with zeros outside,
//            fp32, rintf: within rounding of the float64 value, like the host's torch stage.
//   noise    clip(rint(src + scale z)), z from Philox4x32-10 + Box-Muller addressed by the element index: independent of the launch
//            shape.  A different stream from the same distribution as the host's PCG64 field.
//
// Every product and sum below rounds on its own: contraction is off for the whole file (affine and blur3 are byte-exact only so).
#include "dgp_engine.h"

#include <cmath>
#include <string>

#pragma clang fp contract(off)

namespace dgp {

constexpr int AUG_THREADS = 256;

struct AugFrame {
    const uint8_t* src;
    uint8_t* dst;
    int H, W;
};

__device__ __forceinline__ bool aug_pixel(const AugFrame& f, int* y, int* x) {
    const int p = blockIdx.x * AUG_THREADS + threadIdx.x;       // H * W * 3 < 2^31 (checked on the host)
    if (p >= f.H * f.W) return false;
    *y = p / f.W;
    *x = p - *y * f.W;
    return true;
}

__device__ __forceinline__ uint8_t round_u8(float v) { return (uint8_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

// ---- Pillow's affine_transform + bilinear_filter32RGB (Geometry.c): the sample position of output pixel (x, y) is
// a (x + 0.5) + b (y + 0.5) + c; outside [0, W) x [0, H) the pixel is the fill (0); inside, half a pixel is taken off, the neighbours
// are clamped, a row below the image is replaced by the row itself, and the double result is truncated.
struct AffineArgs {
    AugFrame f;
    double a[6];
};

__global__ __launch_bounds__(AUG_THREADS) void aug_affine_kernel(const AffineArgs p) {
    int y, x;
    if (!aug_pixel(p.f, &y, &x)) return;
    const int H = p.f.H, W = p.f.W;
    const double xc = x + 0.5, yc = y + 0.5;
    double xin = p.a[0] * xc + p.a[1] * yc + p.a[2];
    double yin = p.a[3] * xc + p.a[4] * yc + p.a[5];
    uint8_t* const out = p.f.dst + ((size_t)y * W + x) * 3;
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {       // (a NaN position is outside too)
        out[0] = out[1] = out[2] = 0;
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const int xi = xin < 0.0 ? (int)floor(xin) : (int)xin;
    const int yi = yin < 0.0 ? (int)floor(yin) : (int)yin;
    const double dx = xin - xi, dy = yin - yi;
    const int x0 = min(max(xi, 0), W - 1), x1 = min(max(xi + 1, 0), W - 1);
    const int y0 = min(max(yi, 0), H - 1);
    const bool below = yi + 1 >= 0 && yi + 1 < H;
    const uint8_t* const r0 = p.f.src + (size_t)y0 * W * 3;
    const uint8_t* const r1 = p.f.src + (size_t)(below ? yi + 1 : y0) * W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a0 = r0[x0 * 3 + c], b0 = r0[x1 * 3 + c];
        double v1 = a0 + (b0 - a0) * dx;
        double v2 = v1;
        if (below) {
            const int a1 = r1[x0 * 3 + c], b1 = r1[x1 * 3 + c];
            v2 = a1 + (b1 - a1) * dx;
        }
        v1 = v1 + (v2 - v1) * dy;
        out[c] = (uint8_t)(int)v1;                               // in [0, 255]: a convex combination of bytes
    }
}

// ---- the host's motion blur: out = sum over (yy, xx) of k[2 - yy][2 - xx] * pad[y + yy][x + xx] in fp32, zero weights skipped
struct BlurArgs {
    AugFrame f;
    float k[9];
};

__global__ __launch_bounds__(AUG_THREADS) void aug_blur3_kernel(const BlurArgs p) {
    int y, x;
    if (!aug_pixel(p.f, &y, &x)) return;
    const int H = p.f.H, W = p.f.W;
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int yy = 0; yy < 3; ++yy) {
        const int sy = min(max(y + yy - 1, 0), H - 1);
#pragma unroll
        for (int xx = 0; xx < 3; ++xx) {
            const float w = p.k[(2 - yy) * 3 + (2 - xx)];
            if (w == 0.0f) continue;                             // (uniform over the launch)
            const int sx = min(max(x + xx - 1, 0), W - 1);
            const uint8_t* const s = p.f.src + ((size_t)sy * W + sx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w * (float)s[c];
        }
    }
    uint8_t* const out = p.f.dst + ((size_t)y * W + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = round_u8(acc[c]);
}

// ---- coarse dropout: the coarse cell of pixel (y, x) is (min(y h / H, h - 1), min(x w / W, w - 1)), integer division
struct DropoutArgs {
    AugFrame f;
    const uint8_t* mask;                // [h][w], non-zero: dropped
    int h, w;
};

__global__ __launch_bounds__(AUG_THREADS) void aug_dropout_kernel(const DropoutArgs p) {
    int y, x;
    if (!aug_pixel(p.f, &y, &x)) return;
    const int cy = min((int)(((long long)y * p.h) / p.f.H), p.h - 1);
    const int cx = min((int)(((long long)x * p.w) / p.f.W), p.w - 1);
    const bool drop = p.mask[cy * p.w + cx] != 0;
    const size_t o = ((size_t)y * p.f.W + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) p.f.dst[o + c] = drop ? (uint8_t)0 : p.f.src[o + c];
}

// ---- elastic: field = [2][hc][wc] fp32 (dx then dy), node (i, j) on pixel (4 i, 4 j)
constexpr int AUG_ELASTIC_STEP = 4;

struct ElasticArgs {
    AugFrame f;
    const float* field;
    int hc, wc;
};

__device__ __forceinline__ float coarse_at(const float* g, int wc, int i0, int i1, int j0, int j1, float fy, float fx) {
    const float t0 = g[i0 * wc + j0], t1 = g[i0 * wc + j1], b0 = g[i1 * wc + j0], b1 = g[i1 * wc + j1];
    const float top = t0 + (t1 - t0) * fx, bot = b0 + (b1 - b0) * fx;
    return top + (bot - top) * fy;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_elastic_kernel(const ElasticArgs p) {
    int y, x;
    if (!aug_pixel(p.f, &y, &x)) return;
    const int H = p.f.H, W = p.f.W;
    const int i0 = y / AUG_ELASTIC_STEP, j0 = x / AUG_ELASTIC_STEP;
    const int i1 = min(i0 + 1, p.hc - 1), j1 = min(j0 + 1, p.wc - 1);
    const float fy = (float)(y - i0 * AUG_ELASTIC_STEP) * (1.0f / AUG_ELASTIC_STEP);
    const float fx = (float)(x - j0 * AUG_ELASTIC_STEP) * (1.0f / AUG_ELASTIC_STEP);
    const float dx = coarse_at(p.field, p.wc, i0, i1, j0, j1, fy, fx);
    const float dy = coarse_at(p.field + (size_t)p.hc * p.wc, p.wc, i0, i1, j0, j1, fy, fx);
    uint8_t* const out = p.f.dst + ((size_t)y * W + x) * 3;
    // the sample position is (x + dx, y + dy): the whole pixels are added as integers and the fraction is the shift's own, so the
    // weights carry the shift's precision, not that of a coordinate in the hundreds
    const float fdx = floorf(dx), fdy = floorf(dy);
    const bool sane = fabsf(dx) < 1.0e6f && fabsf(dy) < 1.0e6f;      // (false for a NaN shift too)
    const int xi = sane ? x + (int)fdx : -2, yi = sane ? y + (int)fdy : -2;
    if (xi < -1 || xi > W - 1 || yi < -1 || yi > H - 1) {            // all four neighbours outside
        out[0] = out[1] = out[2] = 0;
        return;
    }
    const float tx = dx - fdx, ty = dy - fdy;                        // in [0, 1]
    const bool l = xi >= 0, r = xi + 1 < W, t = yi >= 0, b = yi + 1 < H;
    const float w00 = (1.0f - tx) * (1.0f - ty), w01 = tx * (1.0f - ty), w10 = (1.0f - tx) * ty, w11 = tx * ty;
    const uint8_t* const r0 = p.f.src + ((size_t)max(yi, 0) * W) * 3;
    const uint8_t* const r1 = p.f.src + ((size_t)min(yi + 1, H - 1) * W) * 3;
    const int xl = max(xi, 0) * 3, xr = min(xi + 1, W - 1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = 0.0f;
        if (t && l) v = v + w00 * (float)r0[xl + c];
        if (t && r) v = v + w01 * (float)r0[xr + c];
        if (b && l) v = v + w10 * (float)r1[xl + c];
        if (b && r) v = v + w11 * (float)r1[xr + c];
        out[c] = round_u8(v);
    }
}

// ---- additive Gaussian noise: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), counter (e / 4, 0, 0, 0), lane e % 4
struct NoiseArgs {
    AugFrame f;
    float scale;
    int per_channel;
    uint32_t key0, key1;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// element e's standard normal: words (0, 1) or (2, 3) of block e / 4 through Box-Muller, cosine for the even lane, sine for the odd one
__device__ __forceinline__ float philox_normal(unsigned long long e, uint32_t k0, uint32_t k1) {
    uint32_t w[4];
    const unsigned long long blk = e >> 2;
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), 0u, 0u, k0, k1, w);
    const int lane = (int)(e & 3);
    const uint32_t wa = lane < 2 ? w[0] : w[2], wb = lane < 2 ? w[1] : w[3];
    const float ua = ((float)(wa >> 8) + 0.5f) * 5.9604644775390625e-08f;          // 2^-24: exact, in (0, 1)
    const float ub = ((float)(wb >> 8) + 0.5f) * 5.9604644775390625e-08f;
    const float rad = sqrtf(-2.0f * logf(ua));
    const float ang = 2.0f * ub;                                  // (exact) in units of pi
    return rad * ((lane & 1) ? sinpif(ang) : cospif(ang));
}

__global__ __launch_bounds__(AUG_THREADS) void aug_noise_kernel(const NoiseArgs p) {
    int y, x;
    if (!aug_pixel(p.f, &y, &x)) return;
    const unsigned long long px = (unsigned long long)y * p.f.W + x;
    const size_t o = (size_t)px * 3;
    float z = 0.0f;
    if (!p.per_channel) z = philox_normal(px, p.key0, p.key1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (p.per_channel) z = philox_normal(px * 3 + c, p.key0, p.key1);
        p.f.dst[o + c] = round_u8((float)p.f.src[o + c] + p.scale * z);
    }
}

// what every entry checks first; `who` names it in the message
static int aug_check(const char* who, const uint8_t* src, uint8_t* dst, int32_t H, int32_t W) {
    const std::string w(who);
    if (!src || !dst) return fail(DGP_ERR_INVALID, w + ": null frame");
    if (H < 2 || W < 2) return fail(DGP_ERR_INVALID, w + ": H and W must be at least 2, got " + std::to_string(H) + " x " + std::to_string(W));
    const long long bytes = (long long)H * W * 3;
    if (bytes > 0x7fffffffLL) return fail(DGP_ERR_INVALID, w + ": a frame of 2 GiB or more");
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    if ((s <= d ? d - s : s - d) < (uintptr_t)bytes) return fail(DGP_ERR_INVALID, w + ": src and dst overlap (the stages do not run in place)");
    return DGP_OK;
}

static dim3 aug_grid(int H, int W) { return dim3((unsigned)(((long long)H * W + AUG_THREADS - 1) / AUG_THREADS)); }

static int aug_launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return DGP_OK;
}

}  // namespace dgp

using namespace dgp;

extern "C" {

int dgp_aug_affine_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const double* coef, void* stream) {
    const int rc = aug_check("dgp_aug_affine_u8", src, dst, H, W);
    if (rc != DGP_OK) return rc;
    if (!coef) return fail(DGP_ERR_INVALID, "dgp_aug_affine_u8: null coefficients");
    AffineArgs a{};
    a.f = AugFrame{src, dst, H, W};
    for (int i = 0; i < 6; ++i) {
        if (!std::isfinite(coef[i])) return fail(DGP_ERR_INVALID, "dgp_aug_affine_u8: coefficient " + std::to_string(i) + " is not finite");
        a.a[i] = coef[i];
    }
    hipLaunchKernelGGL(aug_affine_kernel, aug_grid(H, W), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return aug_launched("dgp_aug_affine_u8");
}

int dgp_aug_blur3_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const float* k, void* stream) {
    const int rc = aug_check("dgp_aug_blur3_u8", src, dst, H, W);
    if (rc != DGP_OK) return rc;
    if (!k) return fail(DGP_ERR_INVALID, "dgp_aug_blur3_u8: null kernel");
    BlurArgs a{};
    a.f = AugFrame{src, dst, H, W};
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(k[i])) return fail(DGP_ERR_INVALID, "dgp_aug_blur3_u8: weight " + std::to_string(i) + " is not finite");
        a.k[i] = k[i];
    }
    hipLaunchKernelGGL(aug_blur3_kernel, aug_grid(H, W), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return aug_launched("dgp_aug_blur3_u8");
}

int dgp_aug_dropout_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const uint8_t* d_mask, int32_t h, int32_t w, void* stream) {
    const int rc = aug_check("dgp_aug_dropout_u8", src, dst, H, W);
    if (rc != DGP_OK) return rc;
    if (!d_mask) return fail(DGP_ERR_INVALID, "dgp_aug_dropout_u8: null mask");
    if (h < 1 || w < 1 || h > H || w > W)
        return fail(DGP_ERR_INVALID, "dgp_aug_dropout_u8: a " + std::to_string(h) + " x " + std::to_string(w) + " mask does not belong to a " +
                                         std::to_string(H) + " x " + std::to_string(W) + " frame (1 .. H by 1 .. W)");
    DropoutArgs a{};
    a.f = AugFrame{src, dst, H, W};
    a.mask = d_mask; a.h = h; a.w = w;
    hipLaunchKernelGGL(aug_dropout_kernel, aug_grid(H, W), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return aug_launched("dgp_aug_dropout_u8");
}

int dgp_aug_elastic_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const float* d_field, int32_t hc, int32_t wc, void* stream) {
    const int rc = aug_check("dgp_aug_elastic_u8", src, dst, H, W);
    if (rc != DGP_OK) return rc;
    if (!d_field) return fail(DGP_ERR_INVALID, "dgp_aug_elastic_u8: null field");
    const int want_h = (H - 1 + AUG_ELASTIC_STEP - 1) / AUG_ELASTIC_STEP + 1, want_w = (W - 1 + AUG_ELASTIC_STEP - 1) / AUG_ELASTIC_STEP + 1;
    if (hc != want_h || wc != want_w)
        return fail(DGP_ERR_INVALID, "dgp_aug_elastic_u8: a " + std::to_string(hc) + " x " + std::to_string(wc) + " field does not belong to a " +
                                         std::to_string(H) + " x " + std::to_string(W) + " frame (" + std::to_string(want_h) + " x " +
                                         std::to_string(want_w) + ")");
    ElasticArgs a{};
    a.f = AugFrame{src, dst, H, W};
    a.field = d_field; a.hc = hc; a.wc = wc;
    hipLaunchKernelGGL(aug_elastic_kernel, aug_grid(H, W), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return aug_launched("dgp_aug_elastic_u8");
}

int dgp_aug_noise_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, float scale, int32_t per_channel, uint64_t key, void* stream) {
    const int rc = aug_check("dgp_aug_noise_u8", src, dst, H, W);
    if (rc != DGP_OK) return rc;
    if (!std::isfinite(scale)) return fail(DGP_ERR_INVALID, "dgp_aug_noise_u8: scale is not finite");
    NoiseArgs a{};
    a.f = AugFrame{src, dst, H, W};
    a.scale = scale;
    a.per_channel = per_channel ? 1 : 0;
    a.key0 = (uint32_t)key;
    a.key1 = (uint32_t)(key >> 32);
    hipLaunchKernelGGL(aug_noise_kernel, aug_grid(H, W), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return aug_launched("dgp_aug_noise_u8");
}

}  // extern "C"
