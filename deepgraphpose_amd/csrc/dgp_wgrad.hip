// Weight gradients of the training step on gfx950: the three reduction-over-pixels GEMM kernels (fp32 MFMA, fp16-split, LDS-DMA on
// H2 copies / H1 tensors) behind wgrad_launch, and the 16-bit tier's fused stem weight gradient behind stem_wgrad_launch.
#include "dgp_train.h"
#include "dgp_device.h"

using namespace dgp;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
constexpr unsigned OOBT = 0xFFFFFFF0u;

__device__ __forceinline__ float4 bload16(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}

// ------------------------------------------------------------------------------------------------
// weight gradient: dWraw[k][co] += sum_m A[m][k] * dY[m][co]   (k = (tap, ci), HWIO order)
// fp32 MFMA with the output tile's rows = k, cols = co and the reduction over pixels m.  LDS images are the
// natural [pixel][k] / [pixel][co] row-major tiles (no transposes): an MFMA operand register is one
// ds_read_b32 of 32 consecutive floats.  The pixel range is split across workgroups (grid.z), partial sums
// are combined with float atomics (256-B wave shapes).
// ------------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* x;       // NHWC [N,H,W,Cin]  (forward input of the conv)
    const float* dy;      // [M, Cdy] masked upstream gradient (M = N*Ho*Wo)
    float* dw;            // [Kchunks*4][Cdy] accumulated
    float* colsum;        // [Cdy] accumulated column sums of dY (d beta / d bias), or nullptr
    int N, H, W, Cin, log2cin4, Ho, Wo, Cdy;
    int KW, stride, dil, pad_t, pad_l, ntaps, kchunks;
    int M, m_per_block;
    unsigned x_bytes, dy_bytes;
    // wgrad_dma only: the operands' fp16 high / low copies (ConvArgs::shadow, same geometry and byte extents as x / dy) and the range
    // slots that decide whether they may be read: previous step (the scale they were written with) and this step (what they hold)
    const void* xs; const void* dys;
    const float *x_prev, *x_cur, *dy_prev, *dy_cur;
    int* fail_flag;       // x is an H2-only tensor (no fp32 twin, x == nullptr): unusable copies raise this flag instead of falling back
};

template <int T>      // tile = 64T (k) x 64T (co); 4 waves as 2 x 2, wave tile 32T x 32T
__device__ __forceinline__ void wgrad_f32_body(const WgradArgs& p) {
    constexpr int BR = 64 * T;               // tile extent (both dims)
    constexpr int CH = BR / 4;               // 16-byte chunks per tile row
    constexpr int NLD = 32 * CH / 256;       // staged chunks per thread per operand (T=1: 2, T=2: 4)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sA = reinterpret_cast<float*>(smem);          // [2][32][BR]
    float* sB = sA + 2 * 32 * BR;                        // [2][32][BR]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int q0 = blockIdx.x * CH;          // first k-chunk of this tile
    const int n0 = blockIdx.y * BR;          // first output column
    const int m_lo = blockIdx.z * p.m_per_block;
    const int m_hi = min(p.M, m_lo + p.m_per_block);
    const int nsteps = (m_hi - m_lo + 31) / 32;
    if (nsteps <= 0) return;
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)p.dy_bytes, 0x00020000);

    // this thread stages chunk `cc` of pixel rows pr + (256/CH)*i
    const int cc = t % CH, pr = t / CH;
    const int q = q0 + cc;
    const int cin4m1 = (p.Cin >> 2) - 1;
    const int tap = q >> p.log2cin4, ch = (q & cin4m1) << 2;
    const bool qok = q < p.kchunks && tap < p.ntaps;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int dh = kh * p.dil - p.pad_t, dw = kw * p.dil - p.pad_l;
    const int cob = n0 + 4 * cc;
    const bool cok = cob < p.Cdy;
    const int HoWo = p.Ho * p.Wo;

    float4 ra[NLD], rb[NLD];
    auto gload = [&](int step) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int m = m_lo + step * 32 + pr + (256 / CH) * i;
            unsigned offa = OOBT, offb = OOBT;
            if (m < m_hi) {
                const int n = m / HoWo, rem = m - n * HoWo;
                const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
                const int hi = ho * p.stride + dh, wi = wo * p.stride + dw;
                if (qok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                    offa = (unsigned)(((n * p.H + hi) * p.W + wi) * p.Cin + ch) << 2;
                if (cok) offb = (unsigned)(m * p.Cdy + cob) << 2;
            }
            ra[i] = bload16(rs_x, offa);
            rb[i] = bload16(rs_dy, offb);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int row = pr + (256 / CH) * i;
            *reinterpret_cast<float4*>(sA + (buf * 32 + row) * BR + 4 * cc) = ra[i];
            *reinterpret_cast<float4*>(sB + (buf * 32 + row) * BR + 4 * cc) = rb[i];
        }
    };
    floatx16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    gload(0);
    lstore(0);
    __syncthreads();
    const bool do_colsum = p.colsum != nullptr && blockIdx.x == 0 && t < BR;     // one k-tile sums dY's columns
    float csum = 0.f;
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) gload(s + 1);
        if (do_colsum) {
            const float* col = sB + buf * 32 * BR + t;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) csum += col[r * BR];
        }
        const float* a_base = sA + buf * 32 * BR + wm * 32 * T + l31;
        const float* b_base = sB + buf * 32 * BR + wn * 32 * T + l31;
#pragma unroll
        for (int pp = 0; pp < 16; ++pp) {
            const int row = 2 * pp + half;
            float af[T], bf[T];
#pragma unroll
            for (int i = 0; i < T; ++i) af[i] = a_base[row * BR + 32 * i];
#pragma unroll
            for (int j = 0; j < T; ++j) bf[j] = b_base[row * BR + 32 * j];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (s + 1 < nsteps) lstore(buf ^ 1);
        __syncthreads();
    }
    if (do_colsum && n0 + t < p.Cdy) atomicAdd(p.colsum + n0 + t, csum);
    // C/D layout: col = lane&31 (co), row = (r&3) + 8*(r>>2) + 4*half (k)
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int co = n0 + wn * 32 * T + 32 * j + l31;
        if (co >= p.Cdy) continue;
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = q0 * 4 + wm * 32 * T + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (k < p.kchunks * 4) atomicAdd(p.dw + (long long)k * p.Cdy + co, acc[i][j][r]);
            }
    }
}

template <int T>
__global__ __launch_bounds__(256) void wgrad_f32(const WgradArgs p) { wgrad_f32_body<T>(p); }

// ------------------------------------------------------------------------------------------------
// Weight gradient on the 16-bit matrix pipe (fp16 high/low split, 3 MFMAs per fp32-class product; the split and the range
// scaling are those of conv_igemm_split_ls, EXPERIMENTS.md section 2).  Same tiling as wgrad_f32<2>: 128 (k) x 128 (co) tile,
// reduction over 32-pixel steps, pixel range split over grid.z, fp32 atomics.  Both MFMA operands want 8 consecutive
// PIXELS of one channel -- a column of the natural [pixel][channel] tile -- so the LDS images stay row-major (fp16 planes,
// 256-byte pixel rows, 16-byte chunks XOR-swizzled) and the operands come in through ds_read_b64_tr_b16, the hardware
// transposed read (scripts/micro/tr_b16.hip checks its lane map): lane 4q+p of a 16-lane group supplies row q / columns
// 4p..4p+3 of a 4 x 16 block and lane i receives column i.
// ------------------------------------------------------------------------------------------------
typedef _Float16 half8t __attribute__((ext_vector_type(8)));
typedef _Float16 half2t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float rng_scale(const float* slots, int lane) {     // 2^(14 - E) for max = m 2^E; 1 for zero / untracked
    const float4 v = reinterpret_cast<const float4*>(slots)[lane];
    float m = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const int be = (int)((__float_as_uint(m) >> 23) & 0xFF);
    if (be == 0 || be == 0xFF) return 1.f;
    int se = 127 + 14 - (be - 127);
    se = se < 1 ? 1 : (se > 254 ? 254 : se);
    return __uint_as_float((unsigned)se << 23);
}

__device__ __forceinline__ void split_hl(const float4 v, const float s, uint2& ph, uint2& pl) {
    // same 10-VALU sequence as split2_f16 (dgp_device.h): h = f16(s x) written into its half of the packed register,
    // r = s x - h exact in fp32 with h read as an fp16 operand, l = f16(r) packed
    unsigned h01, h23;
    float r0, r1, r2, r3;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h01) : "v"(s), "v"(v.x));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h01) : "v"(s), "v"(v.y));
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h23) : "v"(s), "v"(v.z));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h23) : "v"(s), "v"(v.w));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r0) : "v"(s), "v"(v.x), "v"(h01));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r1) : "v"(s), "v"(v.y), "v"(h01));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r2) : "v"(s), "v"(v.z), "v"(h23));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r3) : "v"(s), "v"(v.w), "v"(h23));
    const half2t l01 = {(_Float16)r0, (_Float16)r1}, l23 = {(_Float16)r2, (_Float16)r3};
    ph.x = h01; ph.y = h23;
    pl.x = __builtin_bit_cast(unsigned, l01); pl.y = __builtin_bit_cast(unsigned, l23);
}

struct WgradRanges { const float* x_absmax; const float* dy_absmax; };

// ------------------------------------------------------------------------------------------------
// wgrad_h3p: the weight-gradient tile as an explicit software pipeline.  Diagnostic-build stamps of the plain, non-pipelined version it
// replaced (b4.conv2, cycles per 32-pixel step of 4400): staging-load issue 1630, transposed reads 690, the 24 MFMAs 850, split + LDS stores 1100, barrier 130 -- the
// phases of a wave ran one after the other and the four waves of a workgroup ran them in lock-step, so each shared unit (texture
// addresser, LDS, matrix pipe) was busy in bursts and idle between them (PMC: TA busy 22 %, L2 hit 83 %, L1->L2 latency 173 cycles,
// MFMA busy 23 %).  Here every MFMA is followed by a fixed slice of the other work:
//   first half of a step  : 12 MFMAs on pixel group 0 | transposed reads of group 1 | split + store of the rows loaded one step ago
//   barrier
//   second half           : 12 MFMAs on pixel group 1 | transposed reads of the NEXT step's group 0 | global loads for step + 2
// MFMAs go round the four accumulator blocks (dependent MFMAs are four issues apart).  LDS addresses are 10 lane registers plus
// instruction offsets (the swizzle XOR splits into a lane part and the constants 4 b and h), staging offsets advance by adds.
// ------------------------------------------------------------------------------------------------
template <unsigned OFF>
__device__ __forceinline__ unsigned long long trr(unsigned base) {
    unsigned long long v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(base), "n"(OFF) : "memory");
    return v;
}

struct WgFrag { unsigned long long v[2][2]; };          // [piece hi/lo][pixels 0-3 / 4-7] of one 32-channel block, one k-group

__device__ __forceinline__ half8t wg_op(const WgFrag& f, int pc) {
    const uint4 u = make_uint4((unsigned)f.v[pc][0], (unsigned)(f.v[pc][0] >> 32), (unsigned)f.v[pc][1], (unsigned)(f.v[pc][1] >> 32));
    return __builtin_bit_cast(half8t, u);
}

__global__ __launch_bounds__(256) void wgrad_h3p(const WgradArgs p, const WgradRanges rg) {
    constexpr int CH = 32;
    constexpr unsigned PLANE = 8192u, BUF = 32768u;
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [2 buffers][A hi, A lo, B hi, B lo][32 pixels x 256 B]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int q0 = blockIdx.x * CH;
    const int n0 = blockIdx.y * 128;
    const int m_lo = blockIdx.z * p.m_per_block;
    const int m_hi = min(p.M, m_lo + p.m_per_block);
    const int nsteps = (m_hi - m_lo + 31) / 32;
    if (nsteps <= 0) return;
    const bool pointwise = p.ntaps == 1 && p.stride == 1 && p.pad_t == 0 && p.pad_l == 0 && p.H == p.Ho && p.W == p.Wo;
    // rows at and beyond m_hi read as zeros through the descriptors' range check where the offset grows with the pixel index
    const unsigned x_lim = pointwise ? (unsigned)min((long long)p.x_bytes, (long long)m_hi * p.Cin * 4) : p.x_bytes;
    const unsigned dy_lim = (unsigned)min((long long)p.dy_bytes, (long long)m_hi * p.Cdy * 4);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)x_lim, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)dy_lim, 0x00020000);
    const float sx = rng_scale(rg.x_absmax, lane), sy = rng_scale(rg.dy_absmax, lane);
    const float post = 1.f / (sx * sy);

    const int cc = t % CH, pr = t / CH;           // this thread stages 4-channel chunk cc of pixel rows pr + 8 i
    const int q = q0 + cc;
    const int cin4m1 = (p.Cin >> 2) - 1;
    const int tap = q >> p.log2cin4, ch = (q & cin4m1) << 2;
    const bool qok = q < p.kchunks && tap < p.ntaps;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int dh = kh * p.dil - p.pad_t, dw = kw * p.dil - p.pad_l;
    const int cob = n0 + 4 * cc;
    const bool cok = cob < p.Cdy;
    const int HoWo = p.Ho * p.Wo;

    // staging walkers: byte offsets of this thread's four pixel rows, advanced by 32 pixels per load
    unsigned offb[4], offa[4];
    int whi[4], wwi[4], mleft[4];
    const unsigned stepb = cok ? 32u * (unsigned)p.Cdy * 4u : 0u;
    const unsigned stepa_pw = qok ? 32u * (unsigned)p.Cin * 4u : 0u;
    const int hlim = p.Ho * p.stride + dh, wlim = p.Wo * p.stride + dw;
    const unsigned d_px = (unsigned)(32 * p.stride * p.Cin * 4);
    const unsigned d_row = (unsigned)((p.stride * p.W - p.Wo * p.stride) * p.Cin * 4);
    const unsigned d_img = (unsigned)((p.H * p.W - p.Ho * p.stride * p.W) * p.Cin * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m_lo + pr + 8 * i;
        offb[i] = cok ? (unsigned)(m * p.Cdy + cob) << 2 : OOBT;
        if (pointwise) {
            offa[i] = qok ? (unsigned)(m * p.Cin + ch) << 2 : OOBT;
            whi[i] = wwi[i] = mleft[i] = 0;
        } else {
            const int n = m / HoWo, rem = m - n * HoWo;
            const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
            whi[i] = ho * p.stride + dh;
            wwi[i] = wo * p.stride + dw;
            offa[i] = (unsigned)(((n * p.H + whi[i]) * p.W + wwi[i]) * p.Cin + ch) << 2;
            mleft[i] = m_hi - m;
        }
    }
    float4 ra[4], rb[4];
    auto load_a = [&](int i) {
        if (pointwise) {
            ra[i] = bload16(rs_x, offa[i]);
            offa[i] += stepa_pw;
        } else {
            const bool ok = qok && mleft[i] > 0 && (unsigned)whi[i] < (unsigned)p.H && (unsigned)wwi[i] < (unsigned)p.W;
            ra[i] = bload16(rs_x, ok ? offa[i] : OOBT);
            mleft[i] -= 32;
            wwi[i] += 32 * p.stride;
            offa[i] += d_px;
            while (wwi[i] >= wlim) {
                wwi[i] -= p.Wo * p.stride;
                whi[i] += p.stride;
                offa[i] += d_row;
                if (whi[i] >= hlim) { whi[i] -= p.Ho * p.stride; offa[i] += d_img; }
            }
        }
    };
    auto load_b = [&](int i) {
        rb[i] = bload16(rs_dy, offb[i]);
        offb[i] += stepb;
    };
    float4 cs4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool do_colsum = p.colsum != nullptr && blockIdx.x == 0;

    // LDS store bases (even / odd i): row pr + 8 i, 16-byte chunk cc >> 1 swizzled, 8-byte half cc & 1
    const int lw = (cc >> 1) ^ (((pr & 3) << 2) | (pr >> 2));
    char* wbase[2];
    wbase[0] = smem + 256 * pr + 16 * lw + 8 * (cc & 1);
    wbase[1] = smem + 256 * pr + 16 * (lw ^ 2) + 8 * (cc & 1);
    // transposed-read bases [operand][block b][pixel half h]
    const int g16 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const int f_lane = (qq << 2) | (2 * (g16 >> 1));
    const unsigned rrow = (unsigned)(size_t)smem + 256u * (8 * (g16 >> 1) + qq) + 8u * (pp & 1);
    unsigned rbase[2][2][2];
#pragma unroll
    for (int op = 0; op < 2; ++op) {
        const int L = (8 * (op == 0 ? wm : wn) + 2 * (g16 & 1) + (pp >> 1)) ^ f_lane;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int h = 0; h < 2; ++h) rbase[op][b][h] = rrow + 16u * (unsigned)(L ^ (4 * b) ^ h);
    }

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    WgFrag F0[2][2], F1[2][2];          // [operand][block]

#define WG_FENCE() __builtin_amdgcn_sched_barrier(0)
    // one split + store unit: u < 4 -> x row u (planes 0, 1), else dY row u - 4 (planes 2, 3)
#define WG_UNIT(SB, U)                                                                                               \
    do {                                                                                                             \
        constexpr int i_ = (U) & 3;                                                                                  \
        char* d_ = wbase[i_ & 1] + (SB) * BUF + 2048 * i_ + ((U) < 4 ? 0 : 2 * PLANE);                               \
        uint2 h_, l_;                                                                                                \
        if ((U) < 4) split_hl(ra[i_], sx, h_, l_);                                                                   \
        else {                                                                                                       \
            split_hl(rb[i_], sy, h_, l_);                                                                            \
            if (do_colsum) { cs4.x += rb[i_].x; cs4.y += rb[i_].y; cs4.z += rb[i_].z; cs4.w += rb[i_].w; }           \
        }                                                                                                            \
        *reinterpret_cast<uint2*>(d_) = h_;                                                                          \
        *reinterpret_cast<uint2*>(d_ + PLANE) = l_;                                                                  \
    } while (0)
#define WG_LOAD(U) do { if ((U) < 4) load_a((U) & 3); else load_b((U) & 3); } while (0)
    // read slice R (0..7) of a fragment set: two of its sixteen transposed reads
#define WG_READ2(F, BUFI, KK, R)                                                                                     \
    do {                                                                                                             \
        constexpr int op_ = ((R) >> 2) & 1, b_ = ((R) >> 1) & 1, pc_ = (R) & 1;                                      \
        constexpr unsigned o_ = (BUFI) * BUF + 4096u * (KK) + (2 * op_ + pc_) * PLANE;                               \
        F[op_][b_].v[pc_][0] = trr<o_>(rbase[op_][b_][0]);                                                           \
        F[op_][b_].v[pc_][1] = trr<o_ + 1024u>(rbase[op_][b_][1]);                                                   \
    } while (0)
    // MFMA number G (0..11) of a half step: term G / 4 (lo*hi, hi*lo, hi*hi), block G % 4
#define WG_MMA(F, G)                                                                                                 \
    do {                                                                                                             \
        constexpr int blk_ = (G) & 3, i_ = blk_ >> 1, j_ = blk_ & 1, term_ = (G) >> 2;                               \
        acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg_op(F[0][i_], term_ == 0 ? 1 : 0),                    \
                                                             wg_op(F[1][j_], term_ == 1 ? 1 : 0), acc[i_][j_], 0, 0, 0); \
    } while (0)
#define WG_WAIT_LDS() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

    // prologue: step 0 -> buffer 0, step 1 -> registers, fragments of step 0 / pixel group 0
#pragma unroll
    for (int u = 0; u < 8; ++u) WG_LOAD(u);
    WG_UNIT(0, 0); WG_UNIT(0, 1); WG_UNIT(0, 2); WG_UNIT(0, 3); WG_UNIT(0, 4); WG_UNIT(0, 5); WG_UNIT(0, 6); WG_UNIT(0, 7);
#pragma unroll
    for (int u = 0; u < 8; ++u) WG_LOAD(u);
    __syncthreads();
    WG_READ2(F0, 0, 0, 0); WG_READ2(F0, 0, 0, 1); WG_READ2(F0, 0, 0, 2); WG_READ2(F0, 0, 0, 3);
    WG_READ2(F0, 0, 0, 4); WG_READ2(F0, 0, 0, 5); WG_READ2(F0, 0, 0, 6); WG_READ2(F0, 0, 0, 7);
    WG_WAIT_LDS();
    WG_FENCE();

    // one step on compute buffer CB: stores go to the other buffer, the next step's first fragments come from it
#define WG_STEP(CB)                                                                                                  \
    do {                                                                                                             \
        WG_MMA(F0, 0);  WG_FENCE(); WG_READ2(F1, CB, 1, 0); WG_FENCE();                                              \
        WG_MMA(F0, 1);  WG_FENCE(); WG_READ2(F1, CB, 1, 1); WG_FENCE();                                              \
        WG_MMA(F0, 2);  WG_FENCE(); WG_READ2(F1, CB, 1, 2); WG_FENCE();                                              \
        WG_MMA(F0, 3);  WG_FENCE(); WG_READ2(F1, CB, 1, 3); WG_FENCE();                                              \
        WG_MMA(F0, 4);  WG_FENCE(); WG_READ2(F1, CB, 1, 4); WG_UNIT(1 - (CB), 0); WG_FENCE();                        \
        WG_MMA(F0, 5);  WG_FENCE(); WG_READ2(F1, CB, 1, 5); WG_UNIT(1 - (CB), 1); WG_FENCE();                        \
        WG_MMA(F0, 6);  WG_FENCE(); WG_READ2(F1, CB, 1, 6); WG_UNIT(1 - (CB), 2); WG_FENCE();                        \
        WG_MMA(F0, 7);  WG_FENCE(); WG_READ2(F1, CB, 1, 7); WG_UNIT(1 - (CB), 3); WG_FENCE();                        \
        WG_MMA(F0, 8);  WG_FENCE(); WG_UNIT(1 - (CB), 4); WG_FENCE();                                                \
        WG_MMA(F0, 9);  WG_FENCE(); WG_UNIT(1 - (CB), 5); WG_FENCE();                                                \
        WG_MMA(F0, 10); WG_FENCE(); WG_UNIT(1 - (CB), 6); WG_FENCE();                                                \
        WG_MMA(F0, 11); WG_FENCE(); WG_UNIT(1 - (CB), 7); WG_FENCE();                                                \
        WG_WAIT_LDS();                                                                                               \
        __syncthreads();                                                                                             \
        WG_FENCE();                                                                                                  \
        WG_MMA(F1, 0);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 0); WG_FENCE();                                        \
        WG_MMA(F1, 1);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 1); WG_FENCE();                                        \
        WG_MMA(F1, 2);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 2); WG_FENCE();                                        \
        WG_MMA(F1, 3);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 3); WG_FENCE();                                        \
        WG_MMA(F1, 4);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 4); WG_LOAD(0); WG_FENCE();                            \
        WG_MMA(F1, 5);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 5); WG_LOAD(4); WG_FENCE();                            \
        WG_MMA(F1, 6);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 6); WG_LOAD(1); WG_FENCE();                            \
        WG_MMA(F1, 7);  WG_FENCE(); WG_READ2(F0, 1 - (CB), 0, 7); WG_LOAD(5); WG_FENCE();                            \
        WG_MMA(F1, 8);  WG_FENCE(); WG_LOAD(2); WG_FENCE();                                                          \
        WG_MMA(F1, 9);  WG_FENCE(); WG_LOAD(6); WG_FENCE();                                                          \
        WG_MMA(F1, 10); WG_FENCE(); WG_LOAD(3); WG_FENCE();                                                          \
        WG_MMA(F1, 11); WG_FENCE(); WG_LOAD(7); WG_FENCE();                                                          \
        WG_WAIT_LDS();                                                                                               \
        WG_FENCE();                                                                                                  \
    } while (0)

    for (int s = 0; s < nsteps; s += 2) {
        WG_STEP(0);
        if (s + 1 < nsteps) WG_STEP(1);
    }
#undef WG_STEP
#undef WG_MMA
#undef WG_READ2
#undef WG_LOAD
#undef WG_UNIT
#undef WG_FENCE
#undef WG_WAIT_LDS

    if (do_colsum && cok) {
        atomicAdd(p.colsum + cob, cs4.x); atomicAdd(p.colsum + cob + 1, cs4.y);
        atomicAdd(p.colsum + cob + 2, cs4.z); atomicAdd(p.colsum + cob + 3, cs4.w);
    }
    // C/D layout: col = lane&31 (co), row = (r&3) + 8*(r>>2) + 4*half (k)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = n0 + wn * 64 + 32 * j + l31;
        if (co >= p.Cdy) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = q0 * 4 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (k < p.kchunks * 4) atomicAdd(p.dw + (long long)k * p.Cdy + co, acc[i][j][r] * post);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// wgrad_dma: the 128 x 128 weight-gradient tile with BOTH operands arriving as fp16 high / low cells by LDS-DMA.
// wgrad_h3p's per-step demand (EXPERIMENTS.md section 6a (4)) was four units at 30-45 % each: 8 staging loads + their address walk, the
// fp16 split of 32 values, 16 ds_write_b64, 32 transposed reads and 24 MFMAs per thread.  Here the producers of x and dY have
// already written the split values (ConvArgs::shadow: the H2 cell layout, [pixel][8 channels: 16 B high | 16 B low]), so a step is
// 4 DMA instructions (no VGPR round trip, no VALU, no ds_write), the same transposed reads and the same MFMAs.
//   LDS        4 stages of 16 pixels x [A | B] x 512 B (per pixel row: 16 high chunks, then 16 low chunks; chunk slot XOR-swizzled by
//              f(row) on the SOURCE side -- the DMA destination is lane-linear -- exactly wgrad_h3p's conflict-free image at twice
//              the row pitch).  64 KB: two workgroups per CU.
//   step u     every wave: 4 DMA instructions (2 x 1 KB of A rows, 2 x 1 KB of B rows) of step u + 4 into stage u & 3 (read out during
//              step u - 1); 12 MFMAs (v_mfma_f32_32x32x16_f16, 3 per product) on the fragments of step u, between them the 16
//              transposed reads of step u + 1 from stage (u + 1) & 3; s_waitcnt vmcnt(8) (own loads of step u + 2 have landed);
//              one barrier.  Three steps (48 KB per workgroup) are in flight.
//   validity   the copies were written with scales predicted from the previous step's ranges; every workgroup checks this step's
//              ranges against them (shadow_usable) and, where the prediction failed (first step, a jump of more than 2^5 up or 2^7 down),
//              runs the fp32-MFMA tile on the fp32 tensors instead (same grid, same LDS size) -- slower, never wrong.
// ------------------------------------------------------------------------------------------------
// H1 (round 5, the 16-bit trainer): both operands are H1 tensors IN PLACE -- the retained activation and the gradient tensor themselves, plain
// NHWC fp16 with predicted power-of-two scales, no copies and no fp32 twins.  A pixel row of a stage is 16 cells of 16 bytes (256 B), ONE
// LDS-DMA instruction per operand, wave and step covers four pixel rows (lane >> 4) x 16 chunk positions (lane & 15), the transposed reads
// are the high-piece reads of the H2 image at half the row pitch, and a step is 4 MFMAs (one per product) instead of 12.  A tensor that
// left its predicted range raises fail_flag (the host repeats the step on the parity path): there is nothing to fall back to.
template <bool H1>
__device__ __forceinline__ void wgrad_dma_t(const WgradArgs& p) {
    constexpr unsigned ROW = H1 ? 256u : 512u, OPB = 16u * ROW, STG = 2u * OPB;      // pixel row, one operand of a stage, a stage (H2: 16 KB)
    constexpr unsigned EB = H1 ? 2u : 4u;         // bytes per channel of the operand tensors
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), half = lane >> 5, l31 = lane & 31;
    const float sx = shadow_scale_for(p.x_prev, lane), sy = shadow_scale_for(p.dy_prev, lane);
    if (!(shadow_usable(sx, p.x_cur, lane) && shadow_usable(sy, p.dy_cur, lane))) {
        if (!H1 && p.x && p.dy) wgrad_f32_body<2>(p);
        else if (p.fail_flag && threadIdx.x == 0) atomicOr(p.fail_flag, 2);       // the host repeats the step on fp32 tensors
        return;
    }
    const int wm = wave >> 1, wn = wave & 1;
    const int q0c = blockIdx.x * 16;               // first 8-channel cell of this k-tile
    const int n0 = blockIdx.y * 128;
    const int m_lo = blockIdx.z * p.m_per_block;
    const int m_hi = min(p.M, m_lo + p.m_per_block);
    if (m_hi <= m_lo) return;
    const int nsub = (((m_hi - m_lo + 15) >> 4) + 3) & ~3;      // 16-pixel steps, rounded up to the unroll (rows past m_hi read as zeros)
    const bool pointwise = p.ntaps == 1 && p.stride == 1 && p.pad_t == 0 && p.pad_l == 0 && p.H == p.Ho && p.W == p.Wo;
    const unsigned xb = H1 ? p.x_bytes >> 1 : p.x_bytes, dyb = H1 ? p.dy_bytes >> 1 : p.dy_bytes;
    const unsigned x_lim = pointwise ? (unsigned)min((long long)xb, (long long)m_hi * p.Cin * EB) : xb;
    const unsigned dy_lim = (unsigned)min((long long)dyb, (long long)m_hi * p.Cdy * EB);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.xs), 0, (int)x_lim, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dys), 0, (int)dy_lim, 0x00020000);
    const float post = 1.f / (sx * sy);

    // ---- DMA lane map.  Instruction e (0, 1) of this wave fills stage rows R_e, R_e + 1 with R_e = 4 (2 (wave >> 1) + e) + 2 (wave & 1):
    // lanes 0-31 the first row, 32-63 the second; slot = lane & 31 -> plane (high / low) = slot >> 4, chunk position cs = slot & 15,
    // which holds logical cell cs ^ f(row), f(row) = ((row & 3) << 2) | ((row >> 2) & 3).  e only flips bit 0 of f: the two cells of a
    // lane are neighbours (same tap), its two pixel rows are 4 apart.
    // (H1: one instruction per operand covers rows 4 wave + (lane >> 4), chunk position lane & 15; f(row) = ((lane >> 4) << 2) | wave; e = 0 only)
    const int slot = lane & 31, plane = H1 ? 0 : slot >> 4, cs_ = H1 ? (lane & 15) : (slot & 15);
    const int f0 = H1 ? (((lane >> 4) << 2) | wave) : (((2 * (wave & 1) + half) << 2) | (2 * (wave >> 1)));
    const int row0 = H1 ? 4 * wave + (lane >> 4) : 4 * (2 * (wave >> 1)) + 2 * (wave & 1) + half;      // stage-local pixel row of instruction 0 (H2: instruction 1: + 4)
    constexpr int NE = H1 ? 1 : 2;                // DMA instructions per operand, wave and step
    const int lc8 = p.log2cin4 - 1;                                              // log2(Cin / 8)
    const int kcells = p.kchunks >> 1;
    int cellA[2], cellB[2];
    bool qok[2], cok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = cs_ ^ f0 ^ e;
        cellA[e] = q0c + c; cellB[e] = c;
        qok[e] = cellA[e] < kcells && (cellA[e] >> lc8) < p.ntaps;
        cok[e] = n0 + 8 * c < p.Cdy;
    }
    const int tap = cellA[0] >> lc8;               // (cells c, c ^ 1 lie in the same tap: Cin / 8 is even)
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int dh = kh * p.dil - p.pad_t, dw = kw * p.dil - p.pad_l;
    const int HoWo = p.Ho * p.Wo;
    const int cmask = (1 << lc8) - 1;
    unsigned offa[2], offb[2];
    int whi[2], wwi[2], mleft[2];
    const unsigned stepb = 16u * (unsigned)p.Cdy * EB, stepa_pw = 16u * (unsigned)p.Cin * EB;
    const int hlim = p.Ho * p.stride + dh, wlim = p.Wo * p.stride + dw;
    const unsigned d_px = (unsigned)(16 * p.stride * p.Cin) * EB;
    const unsigned d_row = (unsigned)((p.stride * p.W - p.Wo * p.stride) * p.Cin) * EB;
    const unsigned d_img = (unsigned)((p.H * p.W - p.Ho * p.stride * p.W) * p.Cin) * EB;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int m = m_lo + row0 + 4 * e;
        const unsigned cha = (unsigned)((cellA[e] & cmask) * 8) * EB + 16u * (unsigned)plane;
        offb[e] = cok[e] ? (unsigned)(m * p.Cdy + n0 + 8 * cellB[e]) * EB + 16u * (unsigned)plane : OOBT;
        if (pointwise) {
            offa[e] = qok[e] ? (unsigned)(m * p.Cin) * EB + cha : OOBT;
            whi[e] = wwi[e] = mleft[e] = 0;
        } else {
            const int n = m / HoWo, rem = m - n * HoWo;
            const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
            whi[e] = ho * p.stride + dh;
            wwi[e] = wo * p.stride + dw;
            offa[e] = (unsigned)(((n * p.H + whi[e]) * p.W + wwi[e]) * p.Cin) * EB + cha;
            mleft[e] = m_hi - m;
        }
    }
    typedef __attribute__((address_space(3))) void lds_void;
    char* const dst0 = smem + (unsigned)__builtin_amdgcn_readfirstlane((H1 ? 4 * wave : 4 * (2 * (wave >> 1)) + 2 * (wave & 1)) * (int)ROW);
    // the four DMA instructions of one step into stage ST (A e = 0, A e = 1, B e = 0, B e = 1), then the walkers move on by 16 pixels
    auto dma_a = [&](char* stage, int e) {
        unsigned off;
        if (pointwise) {
            off = offa[e];
            if (qok[e]) offa[e] += stepa_pw;
        } else {
            const bool ok = qok[e] && mleft[e] > 0 && (unsigned)whi[e] < (unsigned)p.H && (unsigned)wwi[e] < (unsigned)p.W;
            off = ok ? offa[e] : OOBT;
            mleft[e] -= 16;
            wwi[e] += 16 * p.stride;
            offa[e] += d_px;
            while (wwi[e] >= wlim) {
                wwi[e] -= p.Wo * p.stride;
                whi[e] += p.stride;
                offa[e] += d_row;
                if (whi[e] >= hlim) { whi[e] -= p.Ho * p.stride; offa[e] += d_img; }
            }
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void*)(stage + e * (4 * ROW)), 16, (int)off, 0, 0, 0);
    };
    auto dma_b = [&](char* stage, int e) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_dy, (lds_void*)(stage + OPB + e * (4 * ROW)), 16, (int)offb[e], 0, 0, 0);
        if (cok[e]) offb[e] += stepb;
    };

    // transposed-read bases [operand][block b][pixel half h] (wgrad_h3p's map at the 512-byte row pitch)
    const int g16 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const int f_lane = (qq << 2) | (2 * (g16 >> 1));
    const unsigned rrow = (unsigned)(size_t)smem + ROW * (unsigned)(8 * (g16 >> 1) + qq) + 8u * (pp & 1);
    unsigned rbase[2][2][2];
#pragma unroll
    for (int op = 0; op < 2; ++op) {
        const int L = (8 * (op == 0 ? wm : wn) + 2 * (g16 & 1) + (pp >> 1)) ^ f_lane;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int h = 0; h < 2; ++h) rbase[op][b][h] = rrow + 16u * (unsigned)(L ^ (4 * b) ^ h);
    }
    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    WgFrag F0[2][2], F1[2][2];          // [operand][block]

    // column sums of dY (d beta), workgroups of the first k-tile only: thread t owns stage row t >> 4, chunk position t & 15
    const bool do_colsum = p.colsum != nullptr && blockIdx.x == 0;
    float cs8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned cs_off = OPB + ROW * (unsigned)(t >> 4) + 16u * (unsigned)(t & 15);
    auto colsum_stage = [&](const char* stage) {
        const half8 h = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(stage + cs_off));
        if constexpr (H1) {
#pragma unroll
            for (int k = 0; k < 8; ++k) cs8[k] += (float)h[k];
        } else {
        const half8 l = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(stage + cs_off + 256));
#pragma unroll
        for (int k = 0; k < 8; ++k) cs8[k] += (float)h[k] + (float)l[k];
        }
    };

#define WD_FENCE() __builtin_amdgcn_sched_barrier(0)
#define WD_READ2(F, ST, R)                                                                                           \
    do {                                                                                                             \
        constexpr int op_ = ((R) >> 2) & 1, b_ = ((R) >> 1) & 1, pc_ = (R) & 1;                                      \
        constexpr unsigned o_ = (ST) * STG + op_ * OPB + pc_ * 256u;                                                 \
        F[op_][b_].v[pc_][0] = trr<o_>(rbase[op_][b_][0]);                                                           \
        F[op_][b_].v[pc_][1] = trr<o_ + 4u * ROW>(rbase[op_][b_][1]);                                                \
    } while (0)
#define WD_MMA(F, G)                                                                                                 \
    do {                                                                                                             \
        constexpr int blk_ = (G) & 3, i_ = blk_ >> 1, j_ = blk_ & 1, term_ = (G) >> 2;                               \
        acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg_op(F[0][i_], term_ == 0 ? 1 : 0),                    \
                                                             wg_op(F[1][j_], term_ == 1 ? 1 : 0), acc[i_][j_], 0, 0, 0); \
    } while (0)

    // prologue: steps 0..3 in flight, steps 0 and 1 landed, fragments of step 0
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        char* st = dst0 + k * STG;
        dma_a(st, 0); if constexpr (!H1) dma_a(st, 1);
        dma_b(st, 0); if constexpr (!H1) dma_b(st, 1);
    }
    if constexpr (H1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    WD_READ2(F0, 0, 0); WD_READ2(F0, 0, 2); WD_READ2(F0, 0, 4); WD_READ2(F0, 0, 6);
    if constexpr (!H1) { WD_READ2(F0, 0, 1); WD_READ2(F0, 0, 3); WD_READ2(F0, 0, 5); WD_READ2(F0, 0, 7); }
    if (do_colsum) colsum_stage(smem);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                  // stage 0 has been read out: step 4 may land in it
    WD_FENCE();

    // one step on the fragments F (step u, u & 3 == S): DMA of step u + 4 into stage S, fragments of step u + 1 from stage S + 1 into Fn
#define WD_STEP(S, F, Fn)                                                                                            \
    do {                                                                                                             \
        constexpr int NS_ = ((S) + 1) & 3;                                                                           \
        char* st_ = dst0 + (S) * STG;                                                                                \
        dma_a(st_, 0); WD_FENCE();                                                                                   \
        WD_MMA(F, 0);  WD_FENCE(); WD_READ2(Fn, NS_, 0); WD_FENCE();                                                 \
        dma_a(st_, 1); WD_FENCE();                                                                                   \
        WD_MMA(F, 1);  WD_FENCE(); WD_READ2(Fn, NS_, 1); WD_FENCE();                                                 \
        dma_b(st_, 0); WD_FENCE();                                                                                   \
        WD_MMA(F, 2);  WD_FENCE(); WD_READ2(Fn, NS_, 2); WD_FENCE();                                                 \
        dma_b(st_, 1); WD_FENCE();                                                                                   \
        WD_MMA(F, 3);  WD_FENCE(); WD_READ2(Fn, NS_, 3); WD_FENCE();                                                 \
        WD_MMA(F, 4);  WD_FENCE(); WD_READ2(Fn, NS_, 4); WD_FENCE();                                                 \
        WD_MMA(F, 5);  WD_FENCE(); WD_READ2(Fn, NS_, 5); WD_FENCE();                                                 \
        WD_MMA(F, 6);  WD_FENCE(); WD_READ2(Fn, NS_, 6); WD_FENCE();                                                 \
        WD_MMA(F, 7);  WD_FENCE(); WD_READ2(Fn, NS_, 7); WD_FENCE();                                                 \
        WD_MMA(F, 8);  WD_FENCE();                                                                                   \
        if (do_colsum) colsum_stage(smem + NS_ * STG);                                                               \
        WD_FENCE();                                                                                                  \
        WD_MMA(F, 9);  WD_FENCE();                                                                                   \
        WD_MMA(F, 10); WD_FENCE();                                                                                   \
        WD_MMA(F, 11); WD_FENCE();                                                                                   \
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");                                                  \
        __builtin_amdgcn_s_barrier();                                                                                \
        WD_FENCE();                                                                                                  \
    } while (0)

    // H1: the same step with half of everything but the barrier: 2 DMA instructions, the 4 high-piece read pairs, 4 MFMAs (high x high)
#define WD_STEP1(S, F, Fn)                                                                                           \
    do {                                                                                                             \
        constexpr int NS_ = ((S) + 1) & 3;                                                                           \
        char* st_ = dst0 + (S) * STG;                                                                                \
        dma_a(st_, 0); WD_FENCE();                                                                                   \
        WD_MMA(F, 8);  WD_FENCE(); WD_READ2(Fn, NS_, 0); WD_FENCE();                                                 \
        dma_b(st_, 0); WD_FENCE();                                                                                   \
        WD_MMA(F, 9);  WD_FENCE(); WD_READ2(Fn, NS_, 2); WD_FENCE();                                                 \
        WD_MMA(F, 10); WD_FENCE(); WD_READ2(Fn, NS_, 4); WD_FENCE();                                                 \
        WD_MMA(F, 11); WD_FENCE(); WD_READ2(Fn, NS_, 6); WD_FENCE();                                                 \
        if (do_colsum) colsum_stage(smem + NS_ * STG);                                                               \
        WD_FENCE();                                                                                                  \
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");                                                  \
        __builtin_amdgcn_s_barrier();                                                                                \
        WD_FENCE();                                                                                                  \
    } while (0)
    for (int u = 0; u < nsub; u += 4) {
        if constexpr (H1) {
            WD_STEP1(0, F0, F1);
            WD_STEP1(1, F1, F0);
            WD_STEP1(2, F0, F1);
            WD_STEP1(3, F1, F0);
        } else {
        WD_STEP(0, F0, F1);
        WD_STEP(1, F1, F0);
        WD_STEP(2, F0, F1);
        WD_STEP(3, F1, F0);
        }
    }
#undef WD_STEP1
#undef WD_STEP
#undef WD_MMA
#undef WD_READ2
#undef WD_FENCE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the loads past the end (zeros) still write LDS

    if (do_colsum) {
        // (the colsum of steps nsub.. read zeros; step 0 was added in the prologue)
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);       // [16 rows][128 columns]
        const int r = t >> 4, c = (t & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
#pragma unroll
        for (int k = 0; k < 8; ++k) red[r * 128 + 8 * c + k] = cs8[k];
        __syncthreads();
        if (t < 128 && n0 + t < p.Cdy) {
            float v = 0.f;
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) v += red[r2 * 128 + t];
            atomicAdd(p.colsum + n0 + t, v / sy);
        }
    }
    // C/D layout: col = lane&31 (co), row = (r&3) + 8*(r>>2) + 4*half (k)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = n0 + wn * 64 + 32 * j + l31;
        if (co >= p.Cdy) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = q0c * 8 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (k < p.kchunks * 4) atomicAdd(p.dw + (long long)k * p.Cdy + co, acc[i][j][r] * post);
            }
    }
}

__global__ __launch_bounds__(256, 2) void wgrad_dma(const WgradArgs p) { wgrad_dma_t<false>(p); }
__global__ __launch_bounds__(256, 2) void wgrad_dma_h1(const WgradArgs p) { wgrad_dma_t<true>(p); }

// ------------------------------------------------------------------------------------------------
// 16-bit tier: the stem's weight gradient with the max-pool's backward fused into its loader (round 5).
//   dW[(kh, kw, c)][co] = sum over conv1 pixels (n, y, x) of  in[n, 2y + kh - 3, 2x + kw - 3, c] * dC1[n, y, x, co]
//   dC1[n, y, x, co]    = sum over the <= 4 pool windows q that hold (y, x) of dPool[n, q, co] * [first maximum of (q, co) is (y, x)]
// The layer-by-layer form wrote dC1 as fp32 (216 MB at 11 frames), read it FOUR times (one per 64-row k-tile of the 64 x 64 fp32 tile) and
// ran on the fp32 matrix pipe: 0.30 ms, the last launch of the pass, + 0.13 ms for the pool's backward and an fp32 copy of dPool.  Here a
// workgroup walks items of 4 conv rows x 32 columns: the centred frame patch (13 x 69 pixels) goes to LDS as fp16, dPool (H1 cells, in
// place) and the first-maximum record of the (up to 4 x 18) pool windows that touch the item go to LDS, dC1 of the item is formed there as fp16
// [co][pixel], and the four waves (one 16-channel column block each) run v_mfma_f32_16x16x32_f16 over all 13 k-blocks (196 rows padded to
// 208) with the reduction over the item's 128 pixels -- dC1 never exists in memory, dPool and the record are read once.  The A operand
// (a k row x 8 pixels of one conv row: stride-2 input columns) is gathered with eight 2-byte LDS reads; a reduction group is 4 rows x 8
// columns so that the four k-groups of a wave read rows 2 * 74 pixels apart (8 banks: conflict-free).  Partial sums stay in registers over
// all items of the (persistent) workgroup and are added to dW with float atomics at the end, scaled by 1 / (dPool's predicted scale).
// ------------------------------------------------------------------------------------------------
constexpr int STEM_SLAB_ROW = 196 * 64 + 64;
struct StemWgradArgs {
    const float* x;              // centred frames [B, H, W, 4] fp32 (preprocess_u8)
    const uint4* g;              // dPool: H1 cells [B, HP, WP, 64]
    const unsigned char* idx;    // first-maximum positions [B, HP, WP, 64]
    const float* g_prev;         // range slots that predict dPool's scale
    float* slab;                 // [gridDim.x][196 x 64 + 64] fp32: every workgroup's partial dW and column sums (plain stores; 512 workgroups
                                 // adding to the SAME 50 KB with float atomics took 2.2 ms: 512 serialized updates per address)
    float* dw;                   // stem_wgrad_reduce_kernel: [49 taps x 4][64] fp32
    float* colsum;               // [64]
    int B, H, W, H1, W1, HP, WP, pt, pl, bands, chunks, nitems;
};

__global__ __launch_bounds__(256) void stem_wgrad_h1_kernel(const StemWgradArgs p) {
    constexpr int IN_R = 13, IN_C = 74, PR = 4, PC = 18, LDY = 136;      // (4 x 18 pool windows: 3 x 17 when the pool's SAME padding starts at 0, one more when it starts at 1)
    typedef float floatx4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) uint2 sIn[IN_R * IN_C];                 // 4 halves per input pixel
    __shared__ __attribute__((aligned(16))) uint4 sG[PR * PC * 8];                  // dPool cells of the item's pool windows
    __shared__ __attribute__((aligned(16))) uint4 sI[PR * PC * 4];                  // their first-maximum bytes
    __shared__ __attribute__((aligned(16))) unsigned short sDy[64 * LDY];           // dC1 of the item, [co][pixel = row * 32 + column]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    floatx4 c[13];
#pragma unroll
    for (int kb = 0; kb < 13; ++kb) c[kb] = floatx4{0.f, 0.f, 0.f, 0.f};
    int kbase[13];                       // half index of this lane's k row inside the patch (-1: padding row)
#pragma unroll
    for (int kb = 0; kb < 13; ++kb) {
        const int kk = 16 * kb + l15, tap = kk >> 2, cc = kk & 3, kh = tap / 7, kw = tap - 7 * kh;
        kbase[kb] = kk < 196 ? (kh * IN_C + kw) * 4 + cc : -1;
    }
    const int o8 = t & 15, co4 = t >> 4;             // dC1 unit of this thread: pixels 8 o8 .. 8 o8 + 7 (one conv row), channels 4 co4 .. + 3
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    const unsigned short* sInH = reinterpret_cast<const unsigned short*>(sIn);
    const unsigned short* sGH = reinterpret_cast<const unsigned short*>(sG);
    const unsigned char* sIB = reinterpret_cast<const unsigned char*>(sI);
    for (int item = blockIdx.x; item < p.nitems; item += gridDim.x) {
        const int n = item / (p.bands * p.chunks), rem = item - n * (p.bands * p.chunks);
        const int y0 = (rem / p.chunks) * 4, x0 = (rem % p.chunks) * 32;
        const int qy0 = (y0 + p.pt) / 2 - 1, qx0 = (x0 + p.pl) / 2 - 1;            // first pool window that can hold (y0, x0)
        // ---- centred frame patch -> fp16
        for (int i = t; i < IN_R * IN_C; i += 256) {
            const int r = i / IN_C, cidx = i - r * IN_C;
            const int gr = 2 * y0 - 3 + r, gc = 2 * x0 - 3 + cidx;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)gr < (unsigned)p.H && (unsigned)gc < (unsigned)p.W)
                v = *reinterpret_cast<const float4*>(p.x + (((size_t)n * p.H + gr) * p.W + gc) * 4);
            const half2v a = {(_Float16)v.x, (_Float16)v.y}, b = {(_Float16)v.z, (_Float16)v.w};
            sIn[i] = make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
        }
        // ---- dPool cells and first-maximum record of the 3 x 17 windows
        for (int i = t; i < PR * PC * 8; i += 256) {
            const int lp = i >> 3, cell = i & 7, a = lp / PC, b = lp - a * PC;
            const int qy = qy0 + a, qx = qx0 + b;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((unsigned)qy < (unsigned)p.HP && (unsigned)qx < (unsigned)p.WP) v = p.g[(((size_t)n * p.HP + qy) * p.WP + qx) * 8 + cell];
            sG[i] = v;
        }
        for (int i = t; i < PR * PC * 4; i += 256) {
            const int lp = i >> 2, part = i & 3, a = lp / PC, b = lp - a * PC;
            const int qy = qy0 + a, qx = qx0 + b;
            uint4 v = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            if ((unsigned)qy < (unsigned)p.HP && (unsigned)qx < (unsigned)p.WP)
                v = *reinterpret_cast<const uint4*>(p.idx + ((((size_t)n * p.HP + qy) * p.WP + qx) * 64 + part * 16));
            sI[i] = v;
        }
        __syncthreads();
        // ---- dC1 of the item: this thread's 8 pixels x 4 channels
        {
            float dy[8][4];
            const int yy = o8 >> 2, xb = (o8 & 3) * 8;
            const int y = y0 + yy;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int x = x0 + xb + e;
                dy[e][0] = dy[e][1] = dy[e][2] = dy[e][3] = 0.f;
                if (y < p.H1 && x < p.W1) {
                    const int qya = max(0, (y + p.pt - 1) / 2), qyb = min(p.HP - 1, (y + p.pt) / 2);
                    const int qxa = max(0, (x + p.pl - 1) / 2), qxb = min(p.WP - 1, (x + p.pl) / 2);
                    for (int qy = qya; qy <= qyb; ++qy)
                        for (int qx = qxa; qx <= qxb; ++qx) {
                            const unsigned me = (unsigned)((y - (2 * qy - p.pt)) * 3 + (x - (2 * qx - p.pl)));
                            const int lp = (qy - qy0) * PC + (qx - qx0);
                            const unsigned k4 = *reinterpret_cast<const unsigned*>(sIB + lp * 64 + 4 * co4);
                            const uint2 g4 = *reinterpret_cast<const uint2*>(sGH + lp * 64 + 4 * co4);
                            const half2v g01 = __builtin_bit_cast(half2v, g4.x), g23 = __builtin_bit_cast(half2v, g4.y);
                            if ((k4 & 0xffu) == me) dy[e][0] += (float)g01[0];
                            if (((k4 >> 8) & 0xffu) == me) dy[e][1] += (float)g01[1];
                            if (((k4 >> 16) & 0xffu) == me) dy[e][2] += (float)g23[0];
                            if ((k4 >> 24) == me) dy[e][3] += (float)g23[1];
                        }
                }
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                unsigned w[4];
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    const half2v h = {(_Float16)dy[2 * e2][cc], (_Float16)dy[2 * e2 + 1][cc]};
                    w[e2] = __builtin_bit_cast(unsigned, h);
                    cs[cc] += (float)h[0] + (float)h[1];
                }
                *reinterpret_cast<uint4*>(sDy + (4 * co4 + cc) * LDY + 8 * o8) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();
        // ---- MFMAs: reduction groups of 4 conv rows (k-group g) x 8 columns
#pragma unroll 1
        for (int blk = 0; blk < 4; ++blk) {
            const uint4 bfrag = *reinterpret_cast<const uint4*>(sDy + (16 * wave + l15) * LDY + 32 * g + 8 * blk);
            const int pbase = ((2 * g) * IN_C + 2 * (8 * blk)) * 4;
#pragma unroll
            for (int kb = 0; kb < 13; ++kb) {
                unsigned w[4] = {0u, 0u, 0u, 0u};
                if (kbase[kb] >= 0) {
                    const unsigned short* q = sInH + kbase[kb] + pbase;
#pragma unroll
                    for (int e2 = 0; e2 < 4; ++e2) w[e2] = (unsigned)q[16 * e2] | ((unsigned)q[16 * e2 + 8] << 16);
                }
                c[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, make_uint4(w[0], w[1], w[2], w[3])),
                                                               __builtin_bit_cast(half8, bfrag), c[kb], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- partial sums -> this workgroup's slab row (column sums: reduced over the 16 threads of a channel quad through LDS first)
    float* row = p.slab + (size_t)blockIdx.x * STEM_SLAB_ROW;
#pragma unroll
    for (int kb = 0; kb < 13; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = 16 * kb + 4 * g + r;
            if (kk < 196) row[kk * 64 + 16 * wave + l15] = c[kb][r];
        }
    float* red = reinterpret_cast<float*>(sDy);          // (free: the last item's MFMAs are behind a barrier)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) red[(4 * co4 + cc) * 16 + o8] = cs[cc];
    __syncthreads();
    if (t < 64) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[t * 16 + k];
        row[196 * 64 + t] = s;
    }
}

// sum of the workgroups' slab rows x 1 / (dPool's predicted scale) -> dW and the column sums (both zeroed by the pass): blockIdx.y sums
// one group of 32 rows with independent loads, the groups meet with float atomics (16-32 per address)
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const StemWgradArgs p, int nrows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float sg = shadow_scale_for(p.g_prev, threadIdx.x & 63);
    if (i >= STEM_SLAB_ROW) return;
    const float inv = sg > 0.f ? 1.f / sg : 0.f;
    const int r0 = blockIdx.y * 32, r1 = min(nrows, r0 + 32);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
        s0 += p.slab[(size_t)r * STEM_SLAB_ROW + i]; s1 += p.slab[(size_t)(r + 1) * STEM_SLAB_ROW + i];
        s2 += p.slab[(size_t)(r + 2) * STEM_SLAB_ROW + i]; s3 += p.slab[(size_t)(r + 3) * STEM_SLAB_ROW + i];
    }
    for (; r < r1; ++r) s0 += p.slab[(size_t)r * STEM_SLAB_ROW + i];
    const float s = ((s0 + s1) + (s2 + s3)) * inv;
    if (i < 196 * 64) atomicAdd(p.dw + i, s);
    else if (p.colsum) atomicAdd(p.colsum + (i - 196 * 64), s);
}

}  // namespace

hipError_t wgrad_launch(const WgradCall& c, hipStream_t s) {
    const dgp_conv_desc& d = c.d;
    const int N = d.N, Cin = d.Cin, Cdy = d.Cout;
    float* const dwraw = c.dwraw; float* const colsum = c.colsum;
    WgradArgs a{};
    a.x = c.x.p; a.dy = c.dy.p; a.dw = dwraw; a.colsum = colsum; a.N = N; a.H = d.H; a.W = d.W; a.Cin = Cin; a.log2cin4 = ilog2(Cin / 4);
    a.Ho = d.Ho; a.Wo = d.Wo; a.Cdy = Cdy; a.KW = d.KW; a.stride = d.stride; a.dil = d.rate; a.pad_t = d.pad_t; a.pad_l = d.pad_l;
    a.ntaps = d.KH * d.KW; a.kchunks = d.KH * d.KW * (Cin / 4); a.M = N * a.Ho * a.Wo;
    const double xb = (double)N * a.H * a.W * Cin * 4, dyb = (double)a.M * Cdy * 4;
    if (!fits_descriptor({xb, dyb})) return hipErrorInvalidValue;
    a.x_bytes = (unsigned)xb;
    a.dy_bytes = (unsigned)dyb;
    hipError_t e = hipSuccess;
    if (c.zeroed) {
        // per-layer scratch, zeroed once for the whole pass (dgp_train_backward)
    } else if (colsum && colsum + 2 * 4096 == dwraw) {      // the plan's layout: [colsum | dot][dwraw] -> one fill
        e = hipMemsetAsync(colsum, 0, ((size_t)2 * 4096 + (size_t)a.kchunks * 4 * Cdy) * sizeof(float), s);
        if (e != hipSuccess) return e;
    } else {
        e = hipMemsetAsync(dwraw, 0, (size_t)a.kchunks * 4 * Cdy * sizeof(float), s);
        if (e != hipSuccess) return e;
        if (colsum) {       // [0, Cdy): column sums, [Cdy, 2 Cdy): dot products of finalize (zeroed together)
            e = hipMemsetAsync(colsum, 0, (size_t)2 * Cdy * sizeof(float), s);
            if (e != hipSuccess) return e;
        }
    }
    const bool h1 = c.h1;
    const bool big = h1 || (a.kchunks * 4 >= 128 && Cdy >= 128);       // (H1 operands: the LDS-DMA tile, partly filled for the 64-channel layers)
    const int BR = big ? 128 : 64;
    const int kt = (a.kchunks * 4 + BR - 1) / BR, nt = (Cdy + BR - 1) / BR;
    // workgroups per launch: ONE round of resident workgroups (2 per CU).  Every workgroup adds its whole 128 x 128 tile to dW with
    // float atomics, so more pixel slices mean more atomic traffic, fewer leave CUs idle: 1536 -> 18.4 ms per step, 1024 -> 17.8,
    // 640 -> 18.2, 512 -> 16.7, 384 -> 17.2, 256 -> 18.1 (DGP_WGRAD_WGS)
    static const int wgs_target = dgp_tune("DGP_WGRAD_WGS", 512);
    static const int wgs_small = dgp_tune("DGP_WGRAD_WGS_SMALL", 1024);      // 64 x 64 tiles: 1024 (16.7 vs 16.9 ms at 512)
    // (wgrad_dma_h1: its loop is shorter, so the 64-KB-per-workgroup atomic epilogue weighs more: 512 -> 7.99, 384 -> 7.80, 256 -> 8.02 ms per step)
    static const int wgs_h1 = dgp_tune("DGP_WGRAD_WGS_H1", 384);
    int split = std::max(1, (h1 ? wgs_h1 : big ? wgs_target : wgs_small) / (kt * nt));
    int mpb = ((a.M + split - 1) / split + 63) / 64 * 64;      // (64: wgrad_dma walks 16-pixel steps unrolled by four)
    if (mpb < 256) mpb = 256;
    split = (a.M + mpb - 1) / mpb;
    a.m_per_block = mpb;
    static const bool h3_env = (dgp_tune("DGP_WGRAD_F16", 1) != 0);       // A/B switch
    const float *rx = c.x.rng, *rdy = c.dy.rng;
    // both operands also exist as fp16 high / low copies written by their producers: LDS-DMA tile (falls back per workgroup to the
    // fp32-MFMA tile when this step's ranges left the copies' predicted scales)
    // (guards: the kernel's offset walkers run up to 15 (row0) + 63 (sub-steps rounded up to four) + 64 (four prefetched steps) = 142
    //  pixel rows past the tensor's end, and its channel masks need Cin / 8 to be a power of two)
    const bool dma_ok = big && g_wgrad_dma && rx && rdy && c.x.cells && c.dy.cells && c.x.prev && c.dy.prev && Cin % 16 == 0 &&
                        ((Cin / 8) & (Cin / 8 - 1)) == 0 && Cdy % 8 == 0 && fits_descriptor({xb + 160.0 * Cin * 4, dyb + 160.0 * Cdy * 4});
    auto read_cells = [&] { a.xs = c.x.cells; a.dys = c.dy.cells; a.x_prev = c.x.prev; a.x_cur = rx; a.dy_prev = c.dy.prev; a.dy_cur = rdy; };
    if (h1) {       // 16-bit tier: both operands are H1 tensors; no other kernel reads them
        if (!(dma_ok && c.fail_flag)) return hipErrorInvalidValue;
        read_cells();
        a.x = nullptr; a.dy = nullptr; a.fail_flag = c.fail_flag;
        hipLaunchKernelGGL(wgrad_dma_h1, dim3(kt, nt, split), dim3(256), 32 * 1024, s, a);
        return hipGetLastError();
    }
    if (dma_ok && h3_env) {
        e = ensure_dynamic_lds<wgrad_dma>(64 * 1024);
        if (e != hipSuccess) return e;
        read_cells();
        if (c.fail_flag) { a.x = nullptr; a.fail_flag = c.fail_flag; }
        hipLaunchKernelGGL(wgrad_dma, dim3(kt, nt, split), dim3(256), 64 * 1024, s, a);
        return hipGetLastError();
    }
    if (c.fail_flag) return hipErrorInvalidValue;          // (no other kernel reads H2 cells)
    if (big && h3_env && rx && rdy && Cin % 4 == 0) {      // both operand ranges known: 16-bit matrix pipe
        e = ensure_dynamic_lds<wgrad_h3p>(64 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(wgrad_h3p, dim3(kt, nt, split), dim3(256), 2 * 4 * 32 * 256, s, a, WgradRanges{rx, rdy});
        return hipGetLastError();
    }
    if (big) {
        e = ensure_dynamic_lds<wgrad_f32<2>>(64 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(wgrad_f32<2>, dim3(kt, nt, split), dim3(256), 2 * 2 * 32 * 128 * 4, s, a);
    } else {
        hipLaunchKernelGGL(wgrad_f32<1>, dim3(kt, nt, split), dim3(256), 2 * 2 * 32 * 64 * 4, s, a);
    }
    return hipGetLastError();
}

// The fused stem weight gradient's two launches (the training step and the layer-level entry point dgp_stem_wgrad_h1): items of 4 conv rows
// x 32 columns over a persistent grid, then the sum of the workgroups' slab rows.  c.slab: one row of STEM_SLAB_ROW floats per workgroup
// (at most one per item).
void stem_wgrad_launch(const StemWgradCall& c, hipStream_t s) {
    StemWgradArgs sa{};
    sa.x = c.x; sa.g = reinterpret_cast<const uint4*>(c.g); sa.idx = c.idx; sa.g_prev = c.g_prev;
    sa.slab = c.slab; sa.dw = c.dw; sa.colsum = c.colsum;
    sa.B = c.B; sa.H = c.H; sa.W = c.W; sa.H1 = c.H1; sa.W1 = c.W1; sa.HP = c.HP; sa.WP = c.WP;
    sa.pt = pool_pad_before(c.H1, c.HP); sa.pl = pool_pad_before(c.W1, c.WP);
    sa.bands = (sa.H1 + 3) / 4; sa.chunks = (sa.W1 + 31) / 32; sa.nitems = sa.B * sa.bands * sa.chunks;
    const int n_cu_s = device_facts().n_cu;
    static const int wgs_per_cu = dgp_tune("DGP_STEM_WGRAD_WGS", 2);      // (1: 6.77, 2: 6.72, 3: 6.72, 4: 6.84 ms per step)
    const int grid = sa.nitems < wgs_per_cu * n_cu_s ? sa.nitems : wgs_per_cu * n_cu_s;
    hipLaunchKernelGGL(stem_wgrad_h1_kernel, dim3((unsigned)grid), dim3(256), 0, s, sa);
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((STEM_SLAB_ROW + 255) / 256, (grid + 31) / 32), dim3(256), 0, s, sa, grid);
}
