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
// The forward direction (dgp_jpeg_forward_u8: frames + markers -> coefficients, for the annotated movie) is described further down.
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

// ---------------------------------------------------------------------------------------------------------------- the forward direction
// RGB frames -> the quantised coefficients libjpeg's baseline encoder computes for them, in the layout dgp_jpeg_entropy_decode writes, so
// that dgp_jpeg_entropy_encode (dgp_jpeg_host.h) makes Pillow's stream of them.  It replaces the draw + encode half of the reference's
// annotated movie (DGP/models/eval.py:46-119).
//
// Launch 1, jpeg_planes_kernel: a thread owns 8 consecutive luma columns of `vs` rows (the pixels under 8 / hs chroma samples of ONE chroma
// row): it reads the pixels with their coordinates clamped to the frame (libjpeg's edge replication: a padded sample is a copy of the last
// real one), lays the enabled markers over them in registers, converts to YCbCr in 16.16 fixed point and stores 8 luma samples per row
// with one 8-byte store and the downsampled chroma with one 4- or 8-byte store per plane.  The whole MCU-padded plane is written, so
// launch 2 never reads a byte nobody wrote.  Chroma rows past the true chroma height repeat the LAST chroma row (pixel rows 2 (ch - 1)
// and 2 (ch - 1) + 1), which for an even H is not what the clamped luma rows are: those threads read their chroma pixels separately.
// Launch 2, jpeg_fdct_kernel: 8 lanes own one block as in jpeg_idct_kernel.  Lane j loads row j (one 8-byte load), runs jfdctint's row
// pass, the intermediate goes through LDS (row pitch 9 dwords, block pitch 72: both the strided and the contiguous access of a 32-lane
// group fall on 32 different banks), lane j runs the column pass on column j and quantises, the int16 results go through LDS once more
// so that lane j stores row j with ONE 16-byte store.  A dummy block (a block of the MCU-padded grid that carries no sample) computes the
// real block whose DC it repeats and keeps only that DC.
struct JpegFwdArgs {
    int B, H, W, hs, vs;
    int blocks_x[3], blocks_y[3], blocks[3], total_blocks;
    int rbx0, rby0;                                // luma blocks that carry samples: ceil(W / 8) x ceil(H / 8) (every chroma block does)
    int ch;                                        // true chroma rows ceil(H / vs)
    int n_markers, dotsize;
    long long src_frame_stride;
};

constexpr int YFIX_R = (int)(0.299 * 65536 + 0.5), YFIX_G = (int)(0.587 * 65536 + 0.5), YFIX_B = (int)(0.114 * 65536 + 0.5);
constexpr int BFIX_R = (int)(0.16874 * 65536 + 0.5), BFIX_G = (int)(0.33126 * 65536 + 0.5), HALF_FIX = (int)(0.5 * 65536 + 0.5);
constexpr int RFIX_G = (int)(0.41869 * 65536 + 0.5), RFIX_B = (int)(0.08131 * 65536 + 0.5);

// pixels [x0, x0 + 8) of row yc (inside the frame), columns clamped to W - 1, with the frame's markers drawn: mk is int32 [n][6] = row,
// col, r, g, b, on; ascending order, so the highest index that covers a pixel wins
__device__ __forceinline__ void load_row8(const uint8_t* __restrict__ frame, const JpegFwdArgs& p, const int32_t* __restrict__ mk, int yc, int x0,
                                          uint8_t (&px)[24]) {
    const uint8_t* const row = frame + (size_t)yc * p.W * 3;
    if (x0 + 8 <= p.W && ((uintptr_t)(row + (size_t)x0 * 3) & 3) == 0) {
        const uint32_t* const r4 = (const uint32_t*)(row + (size_t)x0 * 3);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t v = r4[k];
            px[4 * k] = (uint8_t)v;
            px[4 * k + 1] = (uint8_t)(v >> 8);
            px[4 * k + 2] = (uint8_t)(v >> 16);
            px[4 * k + 3] = (uint8_t)(v >> 24);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint8_t* const q = row + (size_t)min(x0 + k, p.W - 1) * 3;
            px[3 * k] = q[0];
            px[3 * k + 1] = q[1];
            px[3 * k + 2] = q[2];
        }
    }
    if (mk) {
        const long long d = p.dotsize, xa = min(x0, p.W - 1), xb = min(x0 + 7, p.W - 1);
        for (int m = 0; m < p.n_markers; ++m) {
            const int32_t* const e = mk + (size_t)m * 6;
            if (!e[5]) continue;
            const long long r = e[0], c = e[1];
            if (yc < r - d || yc > r + d || xb < c - d || xa > c + d) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long long xc = min(x0 + k, p.W - 1);
                if (xc >= c - d && xc <= c + d) {
                    px[3 * k] = (uint8_t)e[2];
                    px[3 * k + 1] = (uint8_t)e[3];
                    px[3 * k + 2] = (uint8_t)e[4];
                }
            }
        }
    }
}

// grid (ceil(blocks_x[0] * rows / 256), B) with rows = blocks_y[0] * 8 / vs; planes: [B][total_blocks * 64] bytes, Y then Cb then Cr
__global__ __launch_bounds__(256) void jpeg_planes_kernel(const JpegFwdArgs p, const uint8_t* __restrict__ src, const int32_t* __restrict__ markers,
                                                         uint8_t* __restrict__ planes) {
    const int groups = p.blocks_x[0], rows = p.blocks_y[0] * 8 / p.vs;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)groups * rows) return;
    const int ty = (int)(idx / groups), tx = (int)(idx % groups), f = blockIdx.y, x0 = tx * 8;
    const uint8_t* const frame = src + (size_t)f * p.src_frame_stride;
    const int32_t* const mk = markers && p.n_markers > 0 ? markers + (size_t)f * p.n_markers * 6 : nullptr;
    uint8_t* const py = planes + (size_t)f * p.total_blocks * 64;
    uint8_t* const pcb = py + (size_t)p.blocks[0] * 64;
    uint8_t* const pcr = pcb + (size_t)p.blocks[1] * 64;
    const int yp = p.blocks_x[0] * 8, cp = p.blocks_x[1] * 8;
    const bool own_rows = ty < p.ch;               // the chroma row is made of the same pixel rows as the luma rows
    int cb[8], cr[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cb[k] = cr[k] = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (i < p.vs) {
            uint8_t px[24];
            load_row8(frame, p, mk, min(ty * p.vs + i, p.H - 1), x0, px);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int y = (YFIX_R * px[3 * k] + YFIX_G * px[3 * k + 1] + YFIX_B * px[3 * k + 2] + 32768) >> 16;
                if (k < 4) lo |= (uint32_t)y << (8 * k);
                else hi |= (uint32_t)y << (8 * (k - 4));
            }
            *(uint2*)(py + (size_t)(ty * p.vs + i) * yp + x0) = make_uint2(lo, hi);      // a multiple of 8 inside the padded plane
            if (!own_rows) load_row8(frame, p, mk, min((p.ch - 1) * p.vs + i, p.H - 1), x0, px);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
                cb[k] += (-BFIX_R * r - BFIX_G * g + HALF_FIX * b + (128 << 16) + 32767) >> 16;
                cr[k] += (HALF_FIX * r - RFIX_G * g - RFIX_B * b + (128 << 16) + 32767) >> 16;
            }
        }
    }
    if (p.hs == 1) {
        uint32_t blo = 0, bhi = 0, rlo = 0, rhi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            blo |= (uint32_t)cb[k] << (8 * k);
            bhi |= (uint32_t)cb[k + 4] << (8 * k);
            rlo |= (uint32_t)cr[k] << (8 * k);
            rhi |= (uint32_t)cr[k + 4] << (8 * k);
        }
        *(uint2*)(pcb + (size_t)ty * cp + x0) = make_uint2(blo, bhi);
        *(uint2*)(pcr + (size_t)ty * cp + x0) = make_uint2(rlo, rhi);
    } else {
        // jcsample: h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1 ... along the row, h2v2 (a + b + c + d + bias) >> 2 with 1, 2, 1, 2 ...;
        // this thread's first chroma column 4 tx is even
        const int sh = p.vs, base = p.vs - 1;
        uint32_t b4 = 0, r4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b4 |= (uint32_t)((cb[2 * k] + cb[2 * k + 1] + base + (k & 1)) >> sh) << (8 * k);
            r4 |= (uint32_t)((cr[2 * k] + cr[2 * k + 1] + base + (k & 1)) >> sh) << (8 * k);
        }
        *(uint32_t*)(pcb + (size_t)ty * cp + tx * 4) = b4;
        *(uint32_t*)(pcr + (size_t)ty * cp + tx * 4) = r4;
    }
}

// libjpeg's jfdctint ("islow") 1-D pass on d[0..7]; FIRST: the row pass (outputs 0 and 4 scaled up by PASS1_BITS, the rest descaled by
// CONST_BITS - PASS1_BITS), else the column pass (descaled by PASS1_BITS and CONST_BITS + PASS1_BITS)
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int* d, int* o) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15, rnd = 1 << (n - 1);
    if (FIRST) {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + rnd) >> n;
    o[6] = (z1 - t12 * 15137 + rnd) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = (t4 * 2446 + z1 + z3 + rnd) >> n;
    o[5] = (t5 * 16819 + z2 + z4 + rnd) >> n;
    o[3] = (t6 * 25172 + z2 + z3 + rnd) >> n;
    o[1] = (t7 * 12299 + z1 + z4 + rnd) >> n;
}

constexpr int JPG_FWD_ROW_PITCH = 9;               // dwords per block row in LDS: 8 rows = JPG_LDS_PITCH

// grid (ceil(total_blocks / 32), B); planes as jpeg_planes_kernel wrote them; qt: uint16 [2][64]; coef: int16 [B][total_blocks][64]
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const JpegFwdArgs p, const uint8_t* __restrict__ planes, const uint16_t* __restrict__ qt,
                                                       int16_t* __restrict__ coef) {
    __shared__ int ws[JPG_BLOCKS_PER_WG * JPG_LDS_PITCH];
    const int t = threadIdx.x, j = t & 7, lb = t >> 3;
    const int g = blockIdx.x * JPG_BLOCKS_PER_WG + lb;
    const int f = blockIdx.y;
    const bool live = g < p.total_blocks;
    int c = 0, gc = g;
    if (live) {
        if (gc >= p.blocks[0]) { gc -= p.blocks[0]; c = 1; }
        if (c == 1 && gc >= p.blocks[1]) { gc -= p.blocks[1]; c = 2; }
    }
    int* const w = ws + lb * JPG_LDS_PITCH;
    bool dummy = false;
    if (live) {
        const int bx = gc % p.blocks_x[c], by = gc / p.blocks_x[c];
        // the block whose samples count: itself, or for a dummy block the real block its DC chain ends in -- the block before it in MCU
        // order (row-major inside the MCU), followed while that one is dummy too.  Only luma has dummy blocks.
        int sx = bx, sy = by;
        if (c == 0) {
            if (by >= p.rby0) {                    // a dummy row (the MCU's second): back to the end of the MCU's first row
                sy = by - 1;
                sx = bx / p.hs * p.hs + p.hs - 1;
            }
            if (sx >= p.rbx0) sx -= 1;             // a dummy column (the MCU's second)
            dummy = sx != bx || sy != by;
        }
        size_t off = (size_t)f * p.total_blocks * 64;
        if (c >= 1) off += (size_t)p.blocks[0] * 64;
        if (c == 2) off += (size_t)p.blocks[1] * 64;
        off += ((size_t)(sy * 8 + j) * p.blocks_x[c] + sx) * 8;                          // a multiple of 8 inside the plane
        const uint2 v = *(const uint2*)(planes + off);
        int in[8], o[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = (int)((v.x >> (8 * k)) & 255u) - 128;
            in[k + 4] = (int)((v.y >> (8 * k)) & 255u) - 128;
        }
        fdct8<true>(in, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[j * JPG_FWD_ROW_PITCH + k] = o[k];
    }
    __syncthreads();
    int qv[8];
    if (live) {
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = w[r * JPG_FWD_ROW_PITCH + j];
        fdct8<false>(in, o);
        const uint16_t* const q = qt + (c ? 64 : 0);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            // libjpeg: sign(c) ((|c| + (8 q >> 1)) / (8 q)), a truncating divide: an exact unsigned 32-bit division
            const uint32_t d = 8u * max((uint32_t)q[r * 8 + j], 1u);
            const uint32_t a = (uint32_t)abs(o[r]);
            const int m = (int)((a + (d >> 1)) / d);
            qv[r] = o[r] < 0 ? -m : m;
            if (dummy && (r | j) != 0) qv[r] = 0;
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * JPG_FWD_ROW_PITCH + j] = qv[r];
    }
    __syncthreads();
    if (live) {
        uint32_t u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            u[k] = ((uint32_t)w[j * JPG_FWD_ROW_PITCH + 2 * k] & 0xFFFFu) | ((uint32_t)w[j * JPG_FWD_ROW_PITCH + 2 * k + 1] << 16);
        *(uint4*)(coef + ((size_t)f * p.total_blocks + g) * 64 + j * 8) = make_uint4(u[0], u[1], u[2], u[3]);      // 16 bytes, aligned
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

int dgp_jpeg_quality_tables(int32_t quality, uint16_t* qt) {
    if (!qt) return fail(DGP_ERR_INVALID, "dgp_jpeg_quality_tables: null pointer");
    if (!dgp_jpeg::quality_tables(quality, qt)) return fail(DGP_ERR_INVALID, "dgp_jpeg_quality_tables: quality must be in 1..100");
    return DGP_OK;
}

int64_t dgp_jpeg_encode_bound(int32_t H, int32_t W, int32_t sampling) { return dgp_jpeg::encode_bound(H, W, sampling); }

int dgp_jpeg_entropy_encode(const int16_t* coef, int32_t H, int32_t W, int32_t sampling, const uint16_t* qt, uint8_t* out, int64_t cap, int64_t* n) {
    const char* why = "";
    if (!dgp_jpeg::entropy_encode(coef, H, W, sampling, qt, out, cap, n, &why)) return fail(DGP_ERR_INVALID, std::string("dgp_jpeg_entropy_encode: ") + why);
    return DGP_OK;
}

size_t dgp_jpeg_forward_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t sampling) {
    if (sampling == DGP_JPEG_GRAY) return 0;
    return dgp_jpeg_scratch_bytes(B, H, W, sampling);      // the same MCU-padded planes
}

int dgp_jpeg_forward_u8(const uint8_t* src, int32_t B, int32_t H, int32_t W, int64_t src_frame_stride, int32_t sampling, const uint16_t* d_qt,
                        const int32_t* d_markers, int32_t n_markers, int32_t dotsize, int16_t* d_coef, void* scratch, size_t scratch_bytes,
                        void* stream) {
    if (sampling == DGP_JPEG_GRAY)
        return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: grey output is not supported (sampling DGP_JPEG_444, _422 or _420)");
    JpegArgs a;
    const int rc = jpeg_args("dgp_jpeg_forward_u8", B, H, W, sampling, &a);
    if (rc != DGP_OK) return rc;
    if (n_markers < 0 || n_markers > 65535 || dotsize < 0 || dotsize > 65535)
        return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: n_markers and dotsize must be in 0..65535");
    if (B == 0) return DGP_OK;
    if (!src || !d_qt || !d_coef || !scratch) return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: null pointer");
    if (src_frame_stride < (int64_t)H * W * 3) return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: src_frame_stride is less than a frame");
    if (scratch_bytes < (size_t)B * (size_t)a.total_blocks * 64)
        return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: scratch is smaller than dgp_jpeg_forward_scratch_bytes");
    if (((uintptr_t)scratch & 7) != 0) return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: scratch must be 8-byte aligned");
    if (((uintptr_t)d_coef & 15) != 0) return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: d_coef must be 16-byte aligned");
    if (((uintptr_t)d_markers & 3) != 0) return fail(DGP_ERR_INVALID, "dgp_jpeg_forward_u8: d_markers must be 4-byte aligned");
    JpegFwdArgs p{};
    p.B = B; p.H = H; p.W = W;
    p.hs = (sampling == DGP_JPEG_422 || sampling == DGP_JPEG_420) ? 2 : 1;
    p.vs = sampling == DGP_JPEG_420 ? 2 : 1;
    for (int c = 0; c < 3; ++c) {
        p.blocks_x[c] = a.blocks_x[c];
        p.blocks[c] = a.blocks[c];
        p.blocks_y[c] = a.blocks[c] / a.blocks_x[c];
    }
    p.total_blocks = a.total_blocks;
    p.rbx0 = (W + 7) / 8;
    p.rby0 = (H + 7) / 8;
    p.ch = a.ch;
    p.n_markers = d_markers ? n_markers : 0;
    p.dotsize = dotsize;
    p.src_frame_stride = src_frame_stride;
    const long long threads = (long long)p.blocks_x[0] * (p.blocks_y[0] * 8 / p.vs);       // at most 8192 * 65536
    const dim3 g1((unsigned)((threads + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(jpeg_planes_kernel, g1, dim3(256), 0, (hipStream_t)stream, p, src, d_markers, (uint8_t*)scratch);
    const dim3 g2((unsigned)((p.total_blocks + JPG_BLOCKS_PER_WG - 1) / JPG_BLOCKS_PER_WG), (unsigned)B);
    hipLaunchKernelGGL(jpeg_fdct_kernel, g2, dim3(256), 0, (hipStream_t)stream, p, (const uint8_t*)scratch, d_qt, d_coef);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_jpeg_forward_u8: ") + hipGetErrorString(e));
    return DGP_OK;
}

}  // extern "C"
