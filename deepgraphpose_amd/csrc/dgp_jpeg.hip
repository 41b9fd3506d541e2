// gfx950 (MI355X / CDNA4): baseline JPEG reconstruction.  The host (dgp_jpeg_host.h) parses a frame and Huffman-decodes it into quantised
// coefficients; the two kernels here make Pillow's (libjpeg-turbo's) RGB bytes of them.  It replaces the decode half of moviepy's
// VideoFileClip for Motion-JPEG input (DGP/models/eval.py:256) and Pillow's per-frame decode of a directory of JPEGs.
//
// Launch 1, jpeg_idct_kernel: 8 lanes own one 8 x 8 block, a 256-thread workgroup 32 blocks.  Lane j dequantises column j (eight 2-byte
// loads, 16 bytes apart: the 8 lanes of a block cover 16 contiguous bytes per load) and runs libjpeg's "islow" column pass on it, the
// 8 x 8 intermediate goes through LDS (72-dword block pitch: the 32 lanes of a ds_write group fall on 32 different banks), lane j then
// runs the row pass on row j and stores its 8 samples with ONE 8-byte store into the component's plane in scratch.  Planes keep the MCU
// padding (pitch = 8 x blocks per row), so every block store is whole and aligned.
// Launch 2, jpeg_rgb_kernel: a thread owns 4 consecutive pixels of one output row: luma from the plane, chroma through libjpeg's "fancy"
// (triangle) upsampling computed on the TRUE chroma plane size with replicated edges, YCbCr -> RGB in 16.16 fixed point, 12 bytes stored
// as 3 dwords when the address allows it, byte by byte otherwise (odd widths, the ragged last group).  The padding is never read.
// Integer arithmetic only, no atomics, plain vector loads and stores: bit-identical from run to run.  All products fit int32 because the
// host refuses streams with |coefficient x table entry| > 32767.
#include "dgp_engine.h"
#include "dgp_jpeg_host.h"

#include <string>

namespace dgp {

constexpr int JPG_BLOCKS_PER_WG = 32;
constexpr int JPG_LDS_PITCH = 72;          // dwords per block in LDS

struct JpegArgs {
    int B, H, W, sampling, ncomp;
    int blocks_x[3], blocks[3], total_blocks;      // per component: blocks per row of its plane, block count
    int ch, cw;                                    // true chroma plane size: ceil(H v / vmax) x ceil(W h / hmax)
    long long dst_frame_stride;
};

// libjpeg's jidctint ("islow") 1-D pass on i[0..7]: the 8 outputs BEFORE the descale, CONST_BITS = 13
__device__ __forceinline__ void idct8(const int* i, int* o) {
    int z1 = (i[2] + i[6]) * 4433;
    const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const int t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446;
    a1 *= 16819;
    a2 *= 25172;
    a3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    o[0] = t10 + a3; o[7] = t10 - a3;
    o[1] = t11 + a2; o[6] = t11 - a2;
    o[2] = t12 + a1; o[5] = t12 - a1;
    o[3] = t13 + a0; o[4] = t13 - a0;
}

// grid (ceil(total_blocks / 32), B); coef: [B][total_blocks][64] int16, natural order; qt: [B][ncomp][64] uint16; planes: [B][total_blocks * 64] bytes
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegArgs p, const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt,
                                                       uint8_t* __restrict__ planes) {
    __shared__ int ws[JPG_BLOCKS_PER_WG * JPG_LDS_PITCH];
    const int t = threadIdx.x, j = t & 7, lb = t >> 3;
    const int g = blockIdx.x * JPG_BLOCKS_PER_WG + lb;      // block within the frame
    const int f = blockIdx.y;
    const bool live = g < p.total_blocks;
    int c = 0, gc = g;                                       // component, block within the component
    if (live && p.ncomp == 3) {
        if (gc >= p.blocks[0]) { gc -= p.blocks[0]; c = 1; }
        if (c == 1 && gc >= p.blocks[1]) { gc -= p.blocks[1]; c = 2; }
    }
    int* const w = ws + lb * JPG_LDS_PITCH;
    if (live) {
        const int16_t* const cf = coef + ((size_t)f * p.total_blocks + g) * 64;
        const uint16_t* const q = qt + ((size_t)f * p.ncomp + c) * 64;
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (int)cf[r * 8 + j] * (int)q[r * 8 + j];
        idct8(in, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * 8 + j] = (o[r] + (1 << 10)) >> 11;      // CONST_BITS - PASS1_BITS
    }
    __syncthreads();
    if (live) {
        int in[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = w[j * 8 + k];
        idct8(in, o);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = min(max(((o[k] + (1 << 17)) >> 18) + 128, 0), 255);     // CONST_BITS + PASS1_BITS + 3
            if (k < 4) lo |= (uint32_t)v << (8 * k);
            else hi |= (uint32_t)v << (8 * (k - 4));
        }
        const int bx = gc % p.blocks_x[c], by = gc / p.blocks_x[c];
        size_t off = (size_t)f * p.total_blocks * 64;                             // the frame's planes
        if (c >= 1) off += (size_t)p.blocks[0] * 64;
        if (c == 2) off += (size_t)p.blocks[1] * 64;
        off += ((size_t)(by * 8 + j) * p.blocks_x[c] + bx) * 8;                  // multiple of 8: an aligned 8-byte store inside the plane
        *(uint2*)(planes + off) = make_uint2(lo, hi);
    }
}

constexpr int CFIX_R = (int)(1.402 * 65536 + 0.5), CFIX_B = (int)(1.772 * 65536 + 0.5);
constexpr int CFIX_GB = (int)(0.34414 * 65536 + 0.5), CFIX_GR = (int)(0.71414 * 65536 + 0.5);

// one chroma sample at output pixel (y, x) of plane `c` (pitch `cp`, true size ch x cw): libjpeg's fancy upsampling, edges replicated
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ c, int cp, int ch, int cw, int sampling, int y, int x) {
    if (sampling == DGP_JPEG_444) return c[(size_t)y * cp + x];
    const int i = x >> 1;
    const int in = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);      // the neighbour column
    if (sampling == DGP_JPEG_422) {
        const uint8_t* const row = c + (size_t)y * cp;
        return (3 * (int)row[i] + (int)row[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;
    const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);      // the neighbour row
    const uint8_t* const r0 = c + (size_t)r * cp;
    const uint8_t* const r1 = c + (size_t)rn * cp;
    const int cs = 3 * (int)r0[i] + (int)r1[i], csn = 3 * (int)r0[in] + (int)r1[in];
    return (3 * cs + csn + ((x & 1) ? 7 : 8)) >> 4;
}

// grid (ceil(ceil(W / 4) / 64), H, B), 64 threads: thread -> pixels [4 q, 4 q + 4) of row y of frame f
__global__ __launch_bounds__(64) void jpeg_rgb_kernel(const JpegArgs p, const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst) {
    const int q = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    const int x0 = q * 4;
    if (x0 >= p.W) return;
    const uint8_t* const py = planes + (size_t)f * p.total_blocks * 64;
    const int yp = p.blocks_x[0] * 8;
    const uint8_t* const pcb = py + (size_t)p.blocks[0] * 64;
    const uint8_t* const pcr = pcb + (size_t)p.blocks[1] * 64;
    const int cp = p.blocks_x[1] * 8;
    uint8_t px[12];
    const int n = min(4, p.W - x0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(x0 + k, p.W - 1);
        const int yy = py[(size_t)y * yp + x];
        int r = yy, g = yy, b = yy;
        if (p.ncomp == 3) {
            const int cb = chroma_at(pcb, cp, p.ch, p.cw, p.sampling, y, x) - 128;
            const int cr = chroma_at(pcr, cp, p.ch, p.cw, p.sampling, y, x) - 128;
            r = yy + ((CFIX_R * cr + 32768) >> 16);
            b = yy + ((CFIX_B * cb + 32768) >> 16);
            g = yy + ((-CFIX_GB * cb + 32768 - CFIX_GR * cr) >> 16);
        }
        px[3 * k] = (uint8_t)min(max(r, 0), 255);
        px[3 * k + 1] = (uint8_t)min(max(g, 0), 255);
        px[3 * k + 2] = (uint8_t)min(max(b, 0), 255);
    }
    uint8_t* const o = dst + (size_t)f * p.dst_frame_stride + ((size_t)y * p.W + x0) * 3;
    if (n == 4 && ((uintptr_t)o & 3) == 0) {
        uint32_t* const o4 = (uint32_t*)o;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) o[k] = px[k];
    }
}

static int jpeg_args(const char* who, int32_t B, int32_t H, int32_t W, int32_t sampling, JpegArgs* a) {
    dgp_jpeg_info g;
    if (B < 0 || B > 65535) return fail(DGP_ERR_INVALID, std::string(who) + ": 0 to 65535 frames per call");
    if (!dgp_jpeg::geometry(W, H, sampling, &g))
        return fail(DGP_ERR_INVALID, std::string(who) + ": H, W must be in 1..65535 and sampling one of DGP_JPEG_GRAY, _444, _422, _420");
    *a = JpegArgs{};
    a->B = B; a->H = H; a->W = W; a->sampling = sampling; a->ncomp = g.ncomp;
    for (int c = 0; c < 3; ++c) {
        a->blocks_x[c] = g.blocks_x[c];
        a->blocks[c] = g.blocks[c];
    }
    a->total_blocks = g.total_blocks;
    const int hs = (sampling == DGP_JPEG_422 || sampling == DGP_JPEG_420) ? 2 : 1, vs = sampling == DGP_JPEG_420 ? 2 : 1;
    a->ch = (H + vs - 1) / vs;
    a->cw = (W + hs - 1) / hs;
    return DGP_OK;
}

}  // namespace dgp

using namespace dgp;

extern "C" {

int dgp_jpeg_probe(const uint8_t* data, int64_t n, dgp_jpeg_info* info) {
    if (!data || !info || n < 0) return fail(DGP_ERR_INVALID, "dgp_jpeg_probe: null argument");
    dgp_jpeg::State s;
    const char* why = "";
    if (!dgp_jpeg::parse(data, n, &s, &why)) return fail(DGP_ERR_INVALID, std::string("dgp_jpeg_probe: ") + why);
    *info = s.info;
    return DGP_OK;
}

int dgp_jpeg_entropy_decode(const uint8_t* data, int64_t n, const dgp_jpeg_info* info, int16_t* coef, uint16_t* qt) {
    if (!data || n < 0) return fail(DGP_ERR_INVALID, "dgp_jpeg_entropy_decode: null argument");
    const char* why = "";
    if (!dgp_jpeg::entropy_decode(data, n, info, coef, qt, &why)) return fail(DGP_ERR_INVALID, std::string("dgp_jpeg_entropy_decode: ") + why);
    return DGP_OK;
}

size_t dgp_jpeg_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t sampling) {
    JpegArgs a;
    if (jpeg_args("dgp_jpeg_scratch_bytes", B, H, W, sampling, &a) != DGP_OK) return 0;
    return (size_t)B * (size_t)a.total_blocks * 64;
}

int dgp_jpeg_reconstruct_u8(const int16_t* d_coef, const uint16_t* d_qt, int32_t B, int32_t H, int32_t W, int32_t sampling, uint8_t* dst,
                            int64_t dst_frame_stride, void* scratch, size_t scratch_bytes, void* stream) {
    JpegArgs a;
    const int rc = jpeg_args("dgp_jpeg_reconstruct_u8", B, H, W, sampling, &a);
    if (rc != DGP_OK) return rc;
    if (B == 0) return DGP_OK;
    if (!d_coef || !d_qt || !dst || !scratch) return fail(DGP_ERR_INVALID, "dgp_jpeg_reconstruct_u8: null pointer");
    if (dst_frame_stride < (int64_t)H * W * 3) return fail(DGP_ERR_INVALID, "dgp_jpeg_reconstruct_u8: dst_frame_stride is less than a frame");
    if (scratch_bytes < (size_t)B * (size_t)a.total_blocks * 64)
        return fail(DGP_ERR_INVALID, "dgp_jpeg_reconstruct_u8: scratch is smaller than dgp_jpeg_scratch_bytes");
    if (((uintptr_t)scratch & 7) != 0) return fail(DGP_ERR_INVALID, "dgp_jpeg_reconstruct_u8: scratch must be 8-byte aligned");
    a.dst_frame_stride = dst_frame_stride;
    const dim3 g1((unsigned)((a.total_blocks + JPG_BLOCKS_PER_WG - 1) / JPG_BLOCKS_PER_WG), (unsigned)B);
    hipLaunchKernelGGL(jpeg_idct_kernel, g1, dim3(256), 0, (hipStream_t)stream, a, d_coef, d_qt, (uint8_t*)scratch);
    const dim3 g2((unsigned)(((W + 3) / 4 + 63) / 64), (unsigned)H, (unsigned)B);
    hipLaunchKernelGGL(jpeg_rgb_kernel, g2, dim3(64), 0, (hipStream_t)stream, a, (const uint8_t*)scratch, dst);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_jpeg_reconstruct_u8: ") + hipGetErrorString(e));
    return DGP_OK;
}

}  // extern "C"
