// gfx950 (MI355X / CDNA4): Pillow's 8-bit antialiased BICUBIC resample (ImagingResample: what Image.resize(size=...) runs by default)
// and Image.crop after it, as one kernel over a batch of uint8 RGB frames.  It replaces the per-frame PIL resize + crop of
// estimate_pose (DGP/models/eval.py:307-326).  Integer arithmetic on Pillow's own 22-bit coefficient tables: the bytes are Pillow's.
//
// The tables are built on the host (dgp_resize_plan, double arithmetic in Pillow's operation order, contraction off) and handed to
// the kernel as one int32 device array per axis: [out][2] (first input, taps) followed by [out][ksize] coefficients, zero-padded.
//
// resize_crop_kernel: a 192-thread workgroup owns 16 rows x 64 pixels of one frame's output; a thread owns one byte column (pixel,
// channel) of the tile.  It walks the input rows the tile's 16 vertical windows cover, in order: the row segment the 64 horizontal
// windows need is staged in LDS with dword loads (two buffers: row r + 1 is in flight while row r is computed), every thread computes
// its horizontally resampled byte, clips it to uint8 (Pillow stores the horizontal pass as bytes), and adds k_y * byte to the int32
// accumulator of every tile row whose window holds the input row (16 accumulators in registers; the test is uniform over the
// workgroup and the vertical coefficients come through uniform loads).  No intermediate image, no atomics, no scratch; the vertical
// factor is unbounded, the horizontal one by the LDS row buffers (checked on the host before the launch).
//
// dgp_window_resize_u8 runs the same kernel over a WINDOW of one image with Pillow's BOX or BILINEAR tables (dgp_resize_plan_f): crop_image +
// imresize (+ np.fliplr) of the step-0 sample loader.  The window is addressed in place -- ResizeArgs::origin and ::pitch -- and ::mirror
// stores column c at OW - 1 - c.  The tables are clamped to the window, so whatever a dword-staged segment holds beyond it meets zeros only.
#include "dgp_engine.h"

#include <cmath>
#include <string>
#include <vector>

namespace dgp {

constexpr int RSZ_TW = 64;              // output pixels per tile row
constexpr int RSZ_TH = 16;              // output rows per tile
constexpr int RSZ_THREADS = RSZ_TW * 3; // one thread per byte column
constexpr int RSZ_LOADS = 6;            // dwords a thread stages per input row at most
constexpr int RSZ_ROW_DWORDS = RSZ_THREADS * RSZ_LOADS;      // 1152 dwords: an input segment of up to 1534 pixels
constexpr int RSZ_LDS_BYTES = 64 * 1024;
constexpr int RSZ_PRECISION_BITS = 22;

struct ResizeArgs {
    const uint8_t* src;
    uint8_t* dst;
    int H, W, RH, RW, OH, OW;
    int left, upper;                    // output (oy, ox) is pixel (oy + upper, ox + left) of the resized image
    int ksize_x, ksize_y;
    int row_bytes;                      // bytes of one LDS row buffer (multiple of 16)
    // the H x W pixels resampled are a window of a larger image: rows are `pitch` pixels apart, the window's first byte is `origin` bytes
    // into the image and the image (what the descriptor bounds) has `image_bytes` bytes.  Whole frames: W, 0, H * W * 3
    int pitch;
    unsigned origin;
    size_t image_bytes;
    int mirror;                         // output column ox is stored at OW - 1 - ox
};

__device__ __forceinline__ int clip8(int v) { return min(max(v >> RSZ_PRECISION_BITS, 0), 255); }

// plan_x / plan_y: [out][2] bounds, then [out][ksize] coefficients (read-only for the whole launch: uniform indices become scalar loads)
__global__ __launch_bounds__(RSZ_THREADS) void resize_crop_kernel(const ResizeArgs p, const int32_t* __restrict__ plan_x,
                                                                  const int32_t* __restrict__ plan_y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    int32_t* const kx = (int32_t*)(lds + 2 * p.row_bytes);       // [ksize_x][64]: lane-contiguous, conflict-free

    const int t = threadIdx.x;
    const int px = t / 3, ch = t - px * 3;
    const int ox0 = blockIdx.x * RSZ_TW, oy0 = blockIdx.y * RSZ_TH, b = blockIdx.z;
    const int32_t* const bx = plan_x;
    const int32_t* const cx = plan_x + 2 * (long long)p.RW;
    const int32_t* const by = plan_y;
    const int32_t* const cy = plan_y + 2 * (long long)p.RH;

    // ---- the tile's horizontal windows: resized columns [rx_lo, rx_hi) of the 64 (outside the resized image: zeros)
    const int rx_lo = max(ox0 + p.left, 0);
    const int rx_hi = min(min(ox0 + RSZ_TW, p.OW) + p.left, p.RW);
    int seg0 = 0, seg_len = 0;                                   // input pixels [seg0, seg0 + seg_len) of a row
    if (rx_hi > rx_lo) {
        seg0 = bx[2 * rx_lo];
        seg_len = bx[2 * (rx_hi - 1)] + bx[2 * (rx_hi - 1) + 1] - seg0;
    }
    for (int i = t; i < p.ksize_x * RSZ_TW; i += RSZ_THREADS) {
        const int k = i >> 6, q = i & 63;
        const int rx = ox0 + q + p.left;
        kx[i] = (rx >= rx_lo && rx < rx_hi) ? cx[(long long)rx * p.ksize_x + k] : 0;
    }
    const int rx = ox0 + px + p.left;
    const int xoff = (rx >= rx_lo && rx < rx_hi) ? (bx[2 * rx] - seg0) * 3 + ch : 0;      // byte of the thread's first tap in the segment

    // ---- the tile's vertical windows (uniform: scalar registers)
    int ymin[RSZ_TH], yn[RSZ_TH];
    int r0 = p.H, r1 = 0;
#pragma unroll
    for (int yy = 0; yy < RSZ_TH; ++yy) {
        const int ry = oy0 + yy + p.upper;
        const bool in = oy0 + yy < p.OH && ry >= 0 && ry < p.RH;
        ymin[yy] = in ? by[2 * ry] : 0;
        yn[yy] = in ? by[2 * ry + 1] : 0;
        if (in) {
            r0 = min(r0, ymin[yy]);
            r1 = max(r1, ymin[yy] + yn[yy]);
        }
    }
    r0 = max(r0, 0);
    r1 = min(r1, p.H);
    if (seg_len <= 0) r1 = r0;                                   // nothing of the resized image in this tile: zeros

    // ---- source rows through a bounded descriptor of this frame: dword-aligned base (the frame's first byte sits at `mis`) and a whole
    // number of dwords (the range check drops a dword that is only partly inside; the frame's last dword ends inside the same
    // aligned dword as its last byte, so reading it touches no other page)
    const size_t frame_bytes = p.image_bytes;
    const uintptr_t fsrc = (uintptr_t)p.src + (size_t)b * frame_bytes;
    const unsigned mis = (unsigned)(fsrc & 3);
    const __amdgpu_buffer_rsrc_t rs_src =
        __builtin_amdgcn_make_buffer_rsrc((void*)(fsrc - mis), 0, (int)((frame_bytes + mis + 3) & ~(size_t)3), 0x00020000);

    int acc[RSZ_TH];
#pragma unroll
    for (int yy = 0; yy < RSZ_TH; ++yy) acc[yy] = 0;

    uint32_t stage[RSZ_LOADS];
    auto fetch = [&](int r, unsigned* shift) {                   // row r's segment -> registers; *shift: its first byte within the first dword
        const unsigned off = mis + p.origin + ((unsigned)r * (unsigned)p.pitch + (unsigned)seg0) * 3u;
        const unsigned a0 = off & ~3u;
        *shift = off & 3u;
        const int ndw = min((int)((*shift + (unsigned)seg_len * 3u + 3u) >> 2), p.row_bytes >> 2);
#pragma unroll
        for (int i = 0; i < RSZ_LOADS; ++i)
            if (i * RSZ_THREADS < ndw) {
                const int d = i * RSZ_THREADS + t;                   // past ndw: not loaded; past the frame: the descriptor returns 0
                stage[i] = d < ndw ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_src, (int)(a0 + 4u * (unsigned)d), 0, 0) : 0u;
            }
        return ndw;
    };

    unsigned shift = 0, shift_next = 0;
    int ndw = 0, ndw_next = 0;
    if (r0 < r1) ndw_next = fetch(r0, &shift_next);
    int cur = 0;
    for (int r = r0; r < r1; ++r) {
        ndw = ndw_next;
        shift = shift_next;
        uint32_t* const buf = (uint32_t*)(lds + cur * p.row_bytes);      // (an offset into the one LDS array: stays an LDS access)
#pragma unroll
        for (int i = 0; i < RSZ_LOADS; ++i)
            if (i * RSZ_THREADS < ndw) {
                const int d = i * RSZ_THREADS + t;
                if (d < ndw) buf[d] = stage[i];
            }
        __syncthreads();                                         // (also: every thread is done with the buffer written next)
        if (r + 1 < r1) ndw_next = fetch(r + 1, &shift_next);
        // horizontal pass of this thread's byte column, clipped to uint8 as Pillow stores it
        // Every thread runs all ksize_x taps.  A window clipped at a border has fewer (n < ksize_x): its coefficients past n are 0, and the
        // bytes they multiply lie past the staged segment -- stale LDS of an earlier row, the other row buffer or the head of kx.  The read
        // ends at most 3 * ksize_x bytes past a row buffer's staged part and stays inside the allocation only because kx (ksize_x * 256
        // bytes) FOLLOWS the row buffers: keep that order, or bound k by the window's tap count.
        const uint8_t* const rowb = (const uint8_t*)buf + shift + xoff;
        int ss = 1 << (RSZ_PRECISION_BITS - 1);
        for (int k = 0; k < p.ksize_x; ++k) ss += kx[k * RSZ_TW + px] * (int)rowb[3 * k];
        const int hb = clip8(ss);
#pragma unroll
        for (int yy = 0; yy < RSZ_TH; ++yy) {
            const int k = r - ymin[yy];
            if (k >= 0 && k < yn[yy]) acc[yy] += cy[(long long)(oy0 + yy + p.upper) * p.ksize_y + k] * hb;
        }
        cur ^= 1;
    }

    // ---- round, clip, store (ragged tiles predicated; the descriptor bounds the frame's output as well)
    const size_t out_bytes = (size_t)p.OH * p.OW * 3;
    const __amdgpu_buffer_rsrc_t rs_dst = __builtin_amdgcn_make_buffer_rsrc(p.dst + (size_t)b * out_bytes, 0, (int)out_bytes, 0x00020000);
    const int ox = ox0 + px;
    const int oxs = p.mirror ? p.OW - 1 - ox : ox;
#pragma unroll
    for (int yy = 0; yy < RSZ_TH; ++yy) {
        const int oy = oy0 + yy;
        if (oy < p.OH && ox < p.OW) {
            const int v = clip8(acc[yy] + (1 << (RSZ_PRECISION_BITS - 1)));
            __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, rs_dst, (int)(((unsigned)oy * (unsigned)p.OW + (unsigned)oxs) * 3u + (unsigned)ch), 0, 0);
        }
    }
}

// ---- Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter.  Every product and sum below must round on its own:
// a fused multiply-add would change integer coefficients.
#pragma clang fp contract(off)
static double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's box_filter and bilinear_filter
static double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
static double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

static bool filter_known(int filter) { return filter == DGP_FILTER_BOX || filter == DGP_FILTER_BILINEAR || filter == DGP_FILTER_BICUBIC; }
static double filter_support(int filter) { return filter == DGP_FILTER_BOX ? 0.5 : filter == DGP_FILTER_BILINEAR ? 1.0 : 2.0; }

struct AxisGeom {
    double scale, filterscale, support;
    int ksize;
};

static AxisGeom axis_geom(int in_size, int out_size, int filter = DGP_FILTER_BICUBIC) {
    AxisGeom g;
    g.scale = (double)in_size / (double)out_size;
    g.filterscale = g.scale < 1.0 ? 1.0 : g.scale;
    g.support = filter_support(filter) * g.filterscale;
    g.ksize = (int)std::ceil(g.support) * 2 + 1;
    return g;
}

static int plan_check(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0) return fail(DGP_ERR_INVALID, "resize plan: sizes must be positive");
    if (in_size > (1 << 24) || out_size > (1 << 24)) return fail(DGP_ERR_INVALID, "resize plan: size above 2^24");
    return DGP_OK;
}

static void axis_plan(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int filter = DGP_FILTER_BICUBIC) {
#pragma clang fp contract(off)
    const AxisGeom g = axis_geom(in_size, out_size, filter);
    const double ss = 1.0 / g.filterscale;       // BOX, BILINEAR: Pillow's argument (... ) * ss; BICUBIC keeps the division it was pinned with
    std::vector<double> w((size_t)g.ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * g.scale;
        double ww = 0.0;
        int xmin = (int)(center - g.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + g.support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double at = x + xmin - center + 0.5;
            w[x] = filter == DGP_FILTER_BOX ? box_filter(at * ss) : filter == DGP_FILTER_BILINEAR ? bilinear_filter(at * ss)
                                                                                                    : bicubic_filter(at / g.filterscale);
            ww += w[x];
        }
        int32_t* k = coeffs + (size_t)xx * g.ksize;
        for (int x = 0; x < g.ksize; ++x) {
            if (x >= xmax) {
                k[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(v * (double)(1 << RSZ_PRECISION_BITS) - 0.5) : (int32_t)(v * (double)(1 << RSZ_PRECISION_BITS) + 0.5);
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

}  // namespace dgp

using namespace dgp;

extern "C" {

int dgp_resize_plan_size(int32_t in_size, int32_t out_size, int32_t* ksize) {
    const int rc = plan_check(in_size, out_size);
    if (rc != DGP_OK) return rc;
    if (ksize) *ksize = axis_geom(in_size, out_size).ksize;
    return DGP_OK;
}

int dgp_resize_plan(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs) {
    const int rc = plan_check(in_size, out_size);
    if (rc != DGP_OK) return rc;
    if (!bounds || !coeffs) return fail(DGP_ERR_INVALID, "dgp_resize_plan: null bounds or coeffs");
    axis_plan(in_size, out_size, bounds, coeffs);
    return DGP_OK;
}

int dgp_resize_plan_size_f(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize) {
    const int rc = plan_check(in_size, out_size);
    if (rc != DGP_OK) return rc;
    if (!filter_known(filter)) return fail(DGP_ERR_INVALID, "dgp_resize_plan_size_f: filter must be BOX, BILINEAR or BICUBIC");
    if (ksize) *ksize = axis_geom(in_size, out_size, filter).ksize;
    return DGP_OK;
}

int dgp_resize_plan_f(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, int32_t* coeffs) {
    const int rc = plan_check(in_size, out_size);
    if (rc != DGP_OK) return rc;
    if (!filter_known(filter)) return fail(DGP_ERR_INVALID, "dgp_resize_plan_f: filter must be BOX, BILINEAR or BICUBIC");
    if (!bounds || !coeffs) return fail(DGP_ERR_INVALID, "dgp_resize_plan_f: null bounds or coeffs");
    axis_plan(in_size, out_size, bounds, coeffs, filter);
    return DGP_OK;
}

int dgp_resize_crop_u8(const uint8_t* src, int32_t B, int32_t H, int32_t W, int32_t RH, int32_t RW, const int32_t* box, uint8_t* dst,
                       const int32_t* d_plan_x, const int32_t* d_plan_y, int32_t ksize_x, int32_t ksize_y, void* stream) {
    if (B < 0 || H <= 0 || W <= 0 || RH <= 0 || RW <= 0) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: sizes must be positive");
    if (B > 0 && (!src || !dst)) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: null frames");
    if (!d_plan_x || !d_plan_y) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: null plan");
    int rc = plan_check(W, RW);
    if (rc == DGP_OK) rc = plan_check(H, RH);
    if (rc != DGP_OK) return rc;
    const AxisGeom gx = axis_geom(W, RW), gy = axis_geom(H, RH);
    if (ksize_x != gx.ksize || ksize_y != gy.ksize) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: ksize does not belong to these sizes");
    ResizeArgs a{};
    a.left = box ? box[0] : 0;
    a.upper = box ? box[1] : 0;
    const long long ow = box ? (long long)box[2] - box[0] : RW, oh = box ? (long long)box[3] - box[1] : RH;
    if (ow <= 0 || oh <= 0) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: empty crop box");
    if (std::llabs((long long)a.left) > (1 << 24) || std::llabs((long long)a.upper) > (1 << 24) || ow > (1 << 24) || oh > (1 << 24))
        return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: crop box out of range");
    if ((long long)H * W * 3 + 4 > 0x7fffffffLL || oh * ow * 3 > 0x7fffffffLL)
        return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: a frame of 2 GiB or more");
    if (B > 65535) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: more than 65535 frames in one call");
    if (B == 0) return DGP_OK;
    // the input pixels 64 consecutive horizontal windows span: (63 steps of `scale`) + both supports, rounding included
    const long long seg = std::min<long long>(W, (long long)std::ceil(63.0 * gx.scale + 2.0 * gx.support) + 3);
    const long long row_dwords = (seg * 3 + 3 + 3) / 4;
    const long long row_bytes = (row_dwords * 4 + 15) / 16 * 16;
    const long long lds = 2 * row_bytes + (long long)gx.ksize * RSZ_TW * 4;
    if (row_dwords > RSZ_ROW_DWORDS || lds > RSZ_LDS_BYTES)
        return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: the horizontal reduction " + std::to_string(W) + " -> " + std::to_string(RW) +
                                         " needs a row segment beyond the kernel's LDS budget");
    a.src = src;
    a.dst = dst;
    a.H = H; a.W = W; a.RH = RH; a.RW = RW;
    a.OH = (int)oh; a.OW = (int)ow;
    a.ksize_x = ksize_x; a.ksize_y = ksize_y;
    a.row_bytes = (int)row_bytes;
    a.pitch = W;
    a.origin = 0;
    a.image_bytes = (size_t)H * W * 3;
    a.mirror = 0;
    const dim3 grid((unsigned)((ow + RSZ_TW - 1) / RSZ_TW), (unsigned)((oh + RSZ_TH - 1) / RSZ_TH), (unsigned)B);
    if (grid.y > 65535) return fail(DGP_ERR_INVALID, "dgp_resize_crop_u8: output too tall");
    hipLaunchKernelGGL(resize_crop_kernel, grid, dim3(RSZ_THREADS), (size_t)lds, (hipStream_t)stream, a, d_plan_x, d_plan_y);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_resize_crop_u8: ") + hipGetErrorString(e));
    return DGP_OK;
}

int dgp_window_resize_u8(const uint8_t* src, int32_t src_H, int32_t src_W, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t RH,
                         int32_t RW, int32_t filter, int32_t mirror, uint8_t* dst, const int32_t* d_plan_x, const int32_t* d_plan_y,
                         int32_t ksize_x, int32_t ksize_y, void* stream) {
    if (src_H <= 0 || src_W <= 0 || RH <= 0 || RW <= 0) return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: sizes must be positive");
    if (!src || !dst) return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: null image");
    if (!d_plan_x || !d_plan_y) return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: null plan");
    if (!filter_known(filter)) return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: filter must be BOX, BILINEAR or BICUBIC");
    if (x0 < 0 || y0 < 0 || x1 < x0 || y1 < y0 || x1 >= src_W || y1 >= src_H)
        return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: the window must lie inside the image");
    const int H = y1 - y0 + 1, W = x1 - x0 + 1;
    int rc = plan_check(W, RW);
    if (rc == DGP_OK) rc = plan_check(H, RH);
    if (rc == DGP_OK) rc = plan_check(src_H, src_W);
    if (rc != DGP_OK) return rc;
    const AxisGeom gx = axis_geom(W, RW, filter), gy = axis_geom(H, RH, filter);
    if (ksize_x != gx.ksize || ksize_y != gy.ksize)
        return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: ksize does not belong to these sizes and this filter");
    if ((long long)src_H * src_W * 3 + 4 > 0x7fffffffLL || (long long)RH * RW * 3 > 0x7fffffffLL)
        return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: an image of 2 GiB or more");
    // as in dgp_resize_crop_u8: the input pixels 64 consecutive horizontal windows span
    const long long seg = std::min<long long>(W, (long long)std::ceil(63.0 * gx.scale + 2.0 * gx.support) + 3);
    const long long row_dwords = (seg * 3 + 3 + 3) / 4;
    const long long row_bytes = (row_dwords * 4 + 15) / 16 * 16;
    const long long lds = 2 * row_bytes + (long long)gx.ksize * RSZ_TW * 4;
    if (row_dwords > RSZ_ROW_DWORDS || lds > RSZ_LDS_BYTES)
        return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: the horizontal reduction " + std::to_string(W) + " -> " + std::to_string(RW) +
                                         " needs a row segment beyond the kernel's LDS budget");
    ResizeArgs a{};
    a.src = src;
    a.dst = dst;
    a.H = H; a.W = W; a.RH = RH; a.RW = RW;
    a.OH = RH; a.OW = RW;
    a.ksize_x = ksize_x; a.ksize_y = ksize_y;
    a.row_bytes = (int)row_bytes;
    a.pitch = src_W;
    a.origin = ((unsigned)y0 * (unsigned)src_W + (unsigned)x0) * 3u;
    a.image_bytes = (size_t)src_H * src_W * 3;
    a.mirror = mirror ? 1 : 0;
    const dim3 grid((unsigned)((RW + RSZ_TW - 1) / RSZ_TW), (unsigned)((RH + RSZ_TH - 1) / RSZ_TH), 1);
    if (grid.y > 65535) return fail(DGP_ERR_INVALID, "dgp_window_resize_u8: output too tall");
    hipLaunchKernelGGL(resize_crop_kernel, grid, dim3(RSZ_THREADS), (size_t)lds, (hipStream_t)stream, a, d_plan_x, d_plan_y);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_window_resize_u8: ") + hipGetErrorString(e));
    return DGP_OK;
}

}  // extern "C"
