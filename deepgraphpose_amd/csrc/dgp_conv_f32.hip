// gfx950 (MI355X / CDNA4): the fp32 convolution kernels (DGP_CONV_MODE=f32, the Cin < 32 layers and the transposed-conv scatter of
// every mode), their plans and their launchers.  The launch layer (dgp_kernels.hip) reaches them through plan_conv_f32 / launch_conv_f32.
//
//   conv_igemm_f32       implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fma chains), NHWC
//                        activations, k-chunked weight panels, LDS-staged double-buffered tiles, fused BN-affine / bias / residual /
//                        ReLU epilogue, optional transposed-conv phase scatter.  Covers K2, K4-K8 of SURVEY.md 2.3 under DGP_CONV_MODE=f32.
//   conv_igemm_f32_ls    the same with loader / compute wave specialisation
//
// Wavefront = 64 lanes everywhere.  No CUDA-compat shims; this file only targets gfx950.
#include "dgp_conv.h"
#include <cstdio>

namespace dgp {

// ------------------------------------------------------------------------------------
// Implicit-GEMM convolution
//
// GEMM view: out[m][co] = sum_k A[m][k] * Wt[k][co]
//   m  = (n, ho, wo) output pixel, k = (tap, ci) with ci fastest, taps row-major (kh, kw).
// K is walked in steps of BK = 32 floats = 8 chunks of 4 consecutive input channels.
// A chunk q = ks*8 + c maps to tap = q / (Cin/4), channel offset (q % (Cin/4)) * 4, so one
// K-step is one tap when Cin >= 32 and spans 8 taps for the Cin = 4 stem.
//
// MFMA operand trick: v_mfma_f32_32x32x2_f32 takes A[i = lane&31][k = lane>>5]; the order of
// k inside the reduction is free as long as A and B agree, so lanes 0-31 own chunk 2*kc and
// lanes 32-63 chunk 2*kc+1 and fetch their 4 k-values with ONE ds_read_b128; register j of
// both halves then feeds MFMA j.  LDS images are [chunk][row][4 floats]: a 32-lane half
// reads 512 contiguous bytes -> conflict-free ds_read_b128.  The A image pads each chunk
// plane by one 16-byte slot so that the 8 lanes that write one pixel's 8 chunks hit
// different banks.
// ------------------------------------------------------------------------------------

// WIDE = (Cin >= 32): all 8 chunks of a K-step lie in ONE tap, so tap / channel bookkeeping is
// wave-uniform (SALU, advanced incrementally) and each A load costs ~7 VALU ops.  The generic
// path (WIDE = false, used by the 4-channel stem) recomputes the tap per lane.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool WIDE>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void conv_igemm_f32(const ConvArgs p) {
    constexpr int NT = 64 * WAVES_M * WAVES_N;     // threads per workgroup (4 or 8 waves)
    constexpr int WM = BM / WAVES_M;       // wave tile rows
    constexpr int WN = BN / WAVES_N;       // wave tile cols
    constexpr int TM = WM / 32;
    constexpr int TN = WN / 32;
    constexpr int RG = NT / 8;             // pixel rows covered by one staging pass (8 chunks per row)
    constexpr int AROWS = BM / RG;         // A rows staged per thread
    constexpr int BSLOTS = 8 * BN / NT;    // B 16-byte slots staged per thread
    constexpr int LDA = BM + 1;            // slots per chunk plane of A
    constexpr int LDC = WN + 4;            // floats per row of a wave's epilogue staging tile
    static_assert(WAVES_M * WAVES_N == 4 || WAVES_M * WAVES_N == 8, "4 or 8 waves per workgroup");
    static_assert(BSLOTS >= 1 && AROWS >= 1, "tile too small for the workgroup");
    static_assert(WAVES_M * WAVES_N * 32 * LDC * 4 <= (2 * 8 * LDA + 2 * 8 * BN) * 16, "epilogue staging must fit");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* sA = reinterpret_cast<float4*>(smem);     // [2][8][LDA]
    float4* sB = sA + 2 * 8 * LDA;                    // [2][8][BN]

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wave_m0 = (wave / WAVES_N) * WM;
    const int wave_n0 = (wave % WAVES_N) * WN;

    // XCD-aware tile mapping (blocks b and b+8 share an XCD / L2): give each XCD a
    // contiguous range of tile ids; inside it the n-tiles of one m-tile are adjacent so the
    // A tile is fetched into that L2 once.  Bijective for any grid size.
    int tile;
    {
        const int nwg = gridDim.x, b = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = b & 7, loc = b >> 3;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    // split-K (heads only): consecutive tile ids are the K-slices of one output tile
    const int ksplit = p.ksplit > 1 ? p.ksplit : 1;
    const int split = tile % ksplit;
    tile /= ksplit;
    const int nk_loc = p.nk / ksplit;
    const int ks_begin = split * nk_loc, ks_end = ks_begin + nk_loc;
    const int mt = tile / p.ntiles;
    const int nt = tile - mt * p.ntiles;
    const int m0 = mt * BM;
    const int n0 = nt * BN;

    const __amdgpu_buffer_rsrc_t rs_in =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, (int)p.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wpk), 0, (int)p.w_bytes, 0x00020000);

    // ---- per-thread A row bookkeeping -------------------------------------------------
    const int c = t & 7;        // chunk within the K-step
    const int rg = t >> 3;      // 0..RG-1
    int hi0[AROWS], wi0[AROWS], pix0[AROWS], nbase[AROWS];
    const int HoWo = p.Ho * p.Wo;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
        const int m = m0 + rg + RG * i;
        if (m < p.M) {
            const int n = m / HoWo;
            const int rem = m - n * HoWo;
            const int ho = rem / p.Wo;
            const int wo = rem - ho * p.Wo;
            hi0[i] = ho * p.stride - p.pad_t;
            wi0[i] = wo * p.stride - p.pad_l;
            pix0[i] = (n * p.H + hi0[i]) * p.W + wi0[i];
            nbase[i] = n * p.H * p.W;
        } else {
            hi0[i] = -(1 << 28);
            wi0[i] = -(1 << 28);
            pix0[i] = 0;
            nbase[i] = 0;
        }
    }
    const int cin4m1 = (p.Cin >> 2) - 1;
    const unsigned b_lane_off = (unsigned)(t / BN) * ((unsigned)p.CoutP * 16u) + (unsigned)((n0 + (t & (BN - 1))) * 16);
    const unsigned b_row_bytes = (unsigned)p.CoutP * 16u;
    int rowoff[AROWS];          // WIDE: byte offset of (pixel row, lane's chunk) at tap (0,0), channel 0
#pragma unroll
    for (int i = 0; i < AROWS; ++i) rowoff[i] = (pix0[i] * p.Cin + 4 * c) * 4;
    // wave-uniform tap walker (WIDE): K-step ks covers tap w_tap, channels [w_ch, w_ch + 32)
    int w_tap = (ks_begin * 8) >> p.log2cin4;
    int w_ch = ((ks_begin * 8) & cin4m1) << 2;
    int w_kh = w_tap / p.KW, w_kw = w_tap - w_kh * p.KW;

    float4 ra[AROWS];
    float4 rb[BSLOTS];

    auto gload = [&](int ks) {
        if constexpr (WIDE) {
            const int dh = w_kh * p.dil, dw = w_kw * p.dil;
            const int doff = ((dh * p.W + dw) * p.Cin + w_ch) * 4;
            const bool tapok = w_tap < p.ntaps;
            if (p.up == 2) {
                // data-gradient of a stride-2 conv: the input (dY) is read on the zero-stuffed grid, i.e. only
                // where the virtual coordinate is even:  dX[hi] += dY[(hi + pad' + kh' d) / 2] W[kh']
#pragma unroll
                for (int i = 0; i < AROWS; ++i) {
                    const int hv = hi0[i] + dh, wv = wi0[i] + dw;
                    const bool ok = tapok && !((hv | wv) & 1) && (unsigned)(hv >> 1) < (unsigned)p.H &&
                                    (unsigned)(wv >> 1) < (unsigned)p.W;
                    const unsigned off = (unsigned)((nbase[i] + (hv >> 1) * p.W + (wv >> 1)) * p.Cin + w_ch + 4 * c) << 2;
                    ra[i] = buf_load16(rs_in, ok ? off : OOB);
                }
            } else {
#pragma unroll
                for (int i = 0; i < AROWS; ++i) {
                    const int hi = hi0[i] + dh, wi = wi0[i] + dw;
                    const bool ok = tapok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                    ra[i] = buf_load16(rs_in, ok ? (unsigned)(rowoff[i] + doff) : OOB);
                }
            }
            w_ch += 32;
            if (w_ch >= p.Cin) {
                w_ch = 0; ++w_tap;
                if (++w_kw == p.KW) { w_kw = 0; ++w_kh; }
            }
        } else {
            const int q = ks * 8 + c;
            const int tap = q >> p.log2cin4;
            const int ch = (q & cin4m1) << 2;
            const int kh = tap / p.KW;
            const int kw = tap - kh * p.KW;
            const int dh = kh * p.dil, dw = kw * p.dil;
            const bool tapok = tap < p.ntaps;
            const int doff = dh * p.W + dw;
#pragma unroll
            for (int i = 0; i < AROWS; ++i) {
                const int hi = hi0[i] + dh, wi = wi0[i] + dw;
                const bool ok = tapok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                const unsigned off = ok ? ((unsigned)((pix0[i] + doff) * p.Cin + ch) << 2) : OOB;
                ra[i] = buf_load16(rs_in, off);
            }
        }
        const unsigned kbase = (unsigned)(ks * 8) * b_row_bytes;
#pragma unroll
        for (int i = 0; i < BSLOTS; ++i)
            rb[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                        rs_w, (int)b_lane_off, (int)(kbase + (unsigned)(i * (NT / BN)) * b_row_bytes), 0));
    };
    auto lstore = [&](int buf) {
        float4* a = sA + buf * 8 * LDA + c * LDA + rg;
#pragma unroll
        for (int i = 0; i < AROWS; ++i) a[RG * i] = ra[i];
        float4* b = sB + buf * 8 * BN + t;
#pragma unroll
        for (int i = 0; i < BSLOTS; ++i) b[NT * i] = rb[i];
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#ifdef DGP_DIAG
    unsigned long long st0 = 0, st1 = 0, st2 = 0;
#endif
#ifdef DGP_DIAG
    if (p.dbg) st0 = __builtin_amdgcn_s_memtime();
#endif
    gload(ks_begin);
    lstore(0);
    __syncthreads();
#ifdef DGP_DIAG
    if (p.dbg) st1 = __builtin_amdgcn_s_memtime();
#endif
    const int half = lane >> 5;
    const int l31 = lane & 31;
#ifdef DGP_DIAG
    unsigned long long d0, d1, d2, d3, d4, d5, acc_gl = 0, acc_mf = 0, acc_vm = 0, acc_ls = 0, acc_ba = 0;
#endif
    for (int ks = ks_begin; ks < ks_end; ++ks) {
        const int buf = (ks - ks_begin) & 1;
        DIAG_STAMP(d0);
        if (ks + 1 < ks_end) gload(ks + 1);          // in flight under the MFMAs below
        DIAG_STAMP(d1);
        const float4* a_base = sA + buf * 8 * LDA + wave_m0 + l31;
        const float4* b_base = sB + buf * 8 * BN + wave_n0 + l31;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int chunk = 2 * kc + half;
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = a_base[chunk * LDA + 32 * i];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = b_base[chunk * BN + 32 * j];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
        }
        DIAG_STAMP(d2);
#ifdef DGP_DIAG
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        DIAG_STAMP(d3);
#endif
        if (ks + 1 < ks_end) lstore(buf ^ 1);
        DIAG_STAMP(d4);
        __syncthreads();
        DIAG_STAMP(d5);
#ifdef DGP_DIAG
        acc_gl += d1 - d0; acc_mf += d2 - d1; acc_vm += d3 - d2; acc_ls += d4 - d3; acc_ba += d5 - d4;
#endif
    }

#ifdef DGP_DIAG
    if (p.dbg) st2 = __builtin_amdgcn_s_memtime();
#endif
    // ---- epilogue ----------------------------------------------------------------------
    // C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    if (p.out_mode == 1) {
        // transposed-conv phase scatter (heads only: tiny, per-element stores)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int co = n0 + wave_n0 + 32 * j + l31;
            const bool cok = co < p.Cout;
            const float bi = (cok && p.bias && split == 0) ? p.bias[co] : 0.f;
            const int ph = co / p.dc_nj;
            const int cj = co - ph * p.dc_nj;
            const int ph_a = ph >> 1, ph_b = ph & 1;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                    const int m = m0 + wave_m0 + 32 * i + row;
                    if (!cok || m >= p.M) continue;
                    const int n = m / HoWo;
                    const int rem = m - n * HoWo;
                    const int ho = rem / p.Wo;
                    const int wo = rem - ho * p.Wo;
                    const long long oidx =
                        (((long long)n * (2 * p.Ho) + 2 * ho + ph_a) * (2 * p.Wo) + 2 * wo + ph_b) * p.dc_nj + cj;
                    p.out[(long long)split * p.split_stride + oidx] = acc[i][j][r] + bi;
                }
            }
        }
        return;
    }

    // NHWC output: stage each wave's 32 x WN sub-tile through (now free) LDS so that global
    // traffic is 16 B per lane on full rows, with all residual loads of a pass in flight at once.
    float* sC = reinterpret_cast<float*>(smem) + wave * (32 * LDC);
    constexpr int C4 = WN / 4;                 // float4 per staged row
    constexpr int NV = 32 * C4 / 64;           // float4 per lane per pass
    const __amdgpu_buffer_rsrc_t rs_res =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res ? p.res : p.in), 0,
                                          p.res ? (int)p.res_bytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_out =
        __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)p.out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_mask =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.mask ? p.mask : p.in), 0,
                                          p.mask ? (int)p.out_bytes : 0, 0x00020000);
    const int my_c4 = lane % C4;
    const int my_r0 = lane / C4;
    const int co4 = n0 + wave_n0 + 4 * my_c4;
    const bool cok = co4 < p.Cout;
    float4 sc4 = make_float4(1.f, 1.f, 1.f, 1.f), bi4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok && p.scale) sc4 = *reinterpret_cast<const float4*>(p.scale + co4);
    if (cok && p.bias) bi4 = *reinterpret_cast<const float4*>(p.bias + co4);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        __syncthreads();      // previous pass (or the main loop) is done with this LDS
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                sC[row * LDC + 32 * j + l31] = acc[i][j][r];
            }
        __syncthreads();
        unsigned ooff[NV];
        float4 rres[NV], rmask[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int row = my_r0 + v * (64 / C4);
            const int m = m0 + wave_m0 + 32 * i + row;
            const bool ok = cok && m < p.M;
            ooff[v] = ok ? ((unsigned)(m * p.Cout + co4) << 2) : OOB;
            unsigned roff = OOB;
            if (p.res_s == 1) {
                roff = ooff[v];
            } else if (p.res_s == -2 && ok) {        // residual lives on the 2x coarser grid (zero-stuffed upsample)
                const int n = m / HoWo;
                const int rem = m - n * HoWo;
                const int ho = rem / p.Wo;
                const int wo = rem - ho * p.Wo;
                if (!((ho | wo) & 1))
                    roff = (unsigned)(((n * p.res_H + (ho >> 1)) * p.res_W + (wo >> 1)) * p.Cout + co4) << 2;
            } else if (p.res_s > 1 && ok) {
                const int n = m / HoWo;
                const int rem = m - n * HoWo;
                const int ho = rem / p.Wo;
                const int wo = rem - ho * p.Wo;
                roff = (unsigned)(((n * p.res_H + ho * p.res_s) * p.res_W + wo * p.res_s) * p.Cout + co4) << 2;
            }
            rres[v] = buf_load16(rs_res, roff);      // zeros when there is no residual
            rmask[v] = buf_load16(rs_mask, ooff[v]);  // ReLU gate of the backward pass (zeros when unused)
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int row = my_r0 + v * (64 / C4);
            const float4 a = *reinterpret_cast<const float4*>(sC + row * LDC + 4 * my_c4);
            float4 o;
            o.x = a.x * sc4.x + bi4.x + rres[v].x;
            o.y = a.y * sc4.y + bi4.y + rres[v].y;
            o.z = a.z * sc4.z + bi4.z + rres[v].z;
            o.w = a.w * sc4.w + bi4.w + rres[v].w;
            if (p.relu) {
                o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
            }
            if (p.mask) {          // d/dx of ReLU: pass the gradient where the saved activation is positive
                o.x = rmask[v].x > 0.f ? o.x : 0.f; o.y = rmask[v].y > 0.f ? o.y : 0.f;
                o.z = rmask[v].z > 0.f ? o.z : 0.f; o.w = rmask[v].w > 0.f ? o.w : 0.f;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_out, (int)ooff[v], 0, 0);
            if (ooff[v] != OOB) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
        }
    }
    if (p.out_absmax) track_absmax(p.out_absmax, amax, lane, (int)(blockIdx.x * 8u + (threadIdx.x >> 6)));
#ifdef DGP_DIAG
    if (p.dbg && t == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st3 = __builtin_amdgcn_s_memtime();
        unsigned long long* d = p.dbg + 10ull * blockIdx.x;
        d[0] = st1 - st0; d[1] = st2 - st1; d[2] = st3 - st2;
        d[3] = acc_gl; d[4] = acc_mf; d[5] = acc_vm; d[6] = acc_ls; d[7] = acc_ba;
    }
#endif
}

// ------------------------------------------------------------------------------------
// Loader-specialised variant (Cin >= 32, NHWC output): the workgroup has 4 COMPUTE waves (2 x 2 over the tile)
// that only issue ds_read_b128 + MFMA, and 4 LOADER waves that only issue buffer loads + ds_write.  A
// buffer_load costs the issuing wave hundreds of cycles under load (the L2 -> L1 path is the co-bottleneck
// of this kernel, see EXPERIMENTS.md); with the loads on their own waves that stall no longer sits in front of
// the MFMAs, and every load has a whole K-step (8k cycles) in flight before its LDS write.
//   step ks:  compute reads buf[ks&1]      | loaders write buf[(ks+1)&1] (loaded during step ks-1),
//                                          | then issue the loads of step ks+2;   one s_barrier per step.
// ------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(512, 4) void conv_igemm_f32_ls(const ConvArgs p) {
    constexpr int WM = BM / 2, WN = BN / 2;        // compute waves 2 x 2
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int NLT = 256;                       // loader threads
    constexpr int RG = NLT / 8;
    constexpr int AROWS = BM / RG;
    constexpr int BSLOTS = 8 * BN / NLT;
    constexpr int LDA = BM + 1;
    constexpr int LDC = WN + 4;
    static_assert(4 * 32 * LDC * 4 <= (2 * 8 * LDA + 2 * 8 * BN) * 16, "epilogue staging must fit");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* sA = reinterpret_cast<float4*>(smem);     // [2][8][LDA]
    float4* sB = sA + 2 * 8 * LDA;                    // [2][8][BN]

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile;
    {
        const int nwg = gridDim.x, b = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = b & 7, loc = b >> 3;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = tile / p.ntiles;
    const int nt = tile - mt * p.ntiles;
    const int m0 = mt * BM;
    const int n0 = nt * BN;
    const int HoWo = p.Ho * p.Wo;

    if (wave >= 4) {
        // ================================ loader waves ================================
        const int t = threadIdx.x - 256;
        const __amdgpu_buffer_rsrc_t rs_in =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, (int)p.in_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_w =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wpk), 0, (int)p.w_bytes, 0x00020000);
        const int c = t & 7, rg = t >> 3;
        int hi0[AROWS], wi0[AROWS], rowoff[AROWS], nbase[AROWS];
#pragma unroll
        for (int i = 0; i < AROWS; ++i) {
            const int m = m0 + rg + RG * i;
            if (m < p.M) {
                const int n = m / HoWo;
                const int rem = m - n * HoWo;
                const int ho = rem / p.Wo;
                const int wo = rem - ho * p.Wo;
                hi0[i] = ho * p.stride - p.pad_t;
                wi0[i] = wo * p.stride - p.pad_l;
                rowoff[i] = (((n * p.H + hi0[i]) * p.W + wi0[i]) * p.Cin + 4 * c) * 4;
                nbase[i] = n * p.H * p.W;
            } else {
                hi0[i] = -(1 << 28); wi0[i] = -(1 << 28); rowoff[i] = 0; nbase[i] = 0;
            }
        }
        const unsigned b_lane_off = (unsigned)(t / BN) * ((unsigned)p.CoutP * 16u) + (unsigned)((n0 + (t & (BN - 1))) * 16);
        const unsigned b_row_bytes = (unsigned)p.CoutP * 16u;
        int w_kh = 0, w_kw = 0, w_ch = 0, w_tap = 0;
        // two register sets: the loads of step ks+3 are issued while those of step ks+2 are still in flight, so
        // every load has two K-steps to land (one K-step was not enough: the loaders, not the MFMAs, set the pace)
        float4 ra0[AROWS], rb0[BSLOTS], ra1[AROWS], rb1[BSLOTS];
        auto gload = [&](int ks, float4 (&ra)[AROWS], float4 (&rb)[BSLOTS]) {
            const int dh = w_kh * p.dil, dw = w_kw * p.dil;
            const int doff = ((dh * p.W + dw) * p.Cin + w_ch) * 4;
            const bool tapok = w_tap < p.ntaps;
            if (p.up == 2) {
#pragma unroll
                for (int i = 0; i < AROWS; ++i) {
                    const int hv = hi0[i] + dh, wv = wi0[i] + dw;
                    const bool ok = tapok && !((hv | wv) & 1) && (unsigned)(hv >> 1) < (unsigned)p.H &&
                                    (unsigned)(wv >> 1) < (unsigned)p.W;
                    const unsigned off = (unsigned)((nbase[i] + (hv >> 1) * p.W + (wv >> 1)) * p.Cin + w_ch + 4 * c) << 2;
                    ra[i] = buf_load16(rs_in, ok ? off : OOB);
                }
            } else {
#pragma unroll
                for (int i = 0; i < AROWS; ++i) {
                    const int hi = hi0[i] + dh, wi = wi0[i] + dw;
                    const bool ok = tapok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                    ra[i] = buf_load16(rs_in, ok ? (unsigned)(rowoff[i] + doff) : OOB);
                }
            }
            w_ch += 32;
            if (w_ch >= p.Cin) {
                w_ch = 0; ++w_tap;
                if (++w_kw == p.KW) { w_kw = 0; ++w_kh; }
            }
            // the walker is wave-uniform: say so, or hipcc keeps it in VGPRs / scratch behind exec-masked updates
            w_tap = __builtin_amdgcn_readfirstlane(w_tap); w_kw = __builtin_amdgcn_readfirstlane(w_kw);
            w_kh = __builtin_amdgcn_readfirstlane(w_kh); w_ch = __builtin_amdgcn_readfirstlane(w_ch);
            const unsigned kbase = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(ks * 8) * b_row_bytes));
#pragma unroll
            for (int i = 0; i < BSLOTS; ++i)
                rb[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                            rs_w, (int)b_lane_off, (int)(kbase + (unsigned)(i * (NLT / BN)) * b_row_bytes), 0));
        };
        auto lstore = [&](int buf, float4 (&ra)[AROWS], float4 (&rb)[BSLOTS]) {
            float4* a = sA + buf * 8 * LDA + c * LDA + rg;
#pragma unroll
            for (int i = 0; i < AROWS; ++i) a[RG * i] = ra[i];
            float4* b = sB + buf * 8 * BN + t;
#pragma unroll
            for (int i = 0; i < BSLOTS; ++i) b[NLT * i] = rb[i];
        };
        gload(0, ra0, rb0);
        lstore(0, ra0, rb0);
        if (p.nk > 1) gload(1, ra1, rb1);           // set 1 holds odd steps, set 0 even steps
        if (p.nk > 2) gload(2, ra0, rb0);
        __syncthreads();
        for (int ks = 0; ks < p.nk; ks += 2) {
            // step ks (even): publish step ks+1 (set 1), refill it with step ks+3
            if (ks + 1 < p.nk) lstore(1, ra1, rb1);
            if (ks + 3 < p.nk) gload(ks + 3, ra1, rb1);
            __syncthreads();
            if (ks + 1 >= p.nk) break;
            // step ks+1 (odd): publish step ks+2 (set 0), refill it with step ks+4
            if (ks + 2 < p.nk) lstore(0, ra0, rb0);
            if (ks + 4 < p.nk) gload(ks + 4, ra0, rb0);
            __syncthreads();
        }
        return;
    }

    // ================================== compute waves ==================================
    const int wave_m0 = (wave >> 1) * WM;
    const int wave_n0 = (wave & 1) * WN;
    const int half = lane >> 5, l31 = lane & 31;
    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#ifdef DGP_DIAG
    unsigned long long e0, e1, e2, e3, acc_mf = 0, acc_ba = 0;
    DIAG_STAMP(e0);
#endif
    __syncthreads();
#ifdef DGP_DIAG
    DIAG_STAMP(e1);
    const unsigned long long t_pro = e1 - e0;
#endif
    for (int ks = 0; ks < p.nk; ++ks) {
        const int buf = ks & 1;
        const float4* a_base = sA + buf * 8 * LDA + wave_m0 + l31;
        const float4* b_base = sB + buf * 8 * BN + wave_n0 + l31;
        DIAG_STAMP(e1);
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int chunk = 2 * kc + half;
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = a_base[chunk * LDA + 32 * i];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = b_base[chunk * BN + 32 * j];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
        }
        DIAG_STAMP(e2);
        __syncthreads();
        DIAG_STAMP(e3);
#ifdef DGP_DIAG
        acc_mf += e2 - e1; acc_ba += e3 - e2;
#endif
    }
#ifdef DGP_DIAG
    if (p.dbg && threadIdx.x == 0) {
        unsigned long long* d = p.dbg + 10ull * blockIdx.x;
        d[0] = t_pro; d[1] = acc_mf + acc_ba; d[2] = 0; d[3] = 0; d[4] = acc_mf; d[5] = 0; d[6] = 0; d[7] = acc_ba;
    }
#endif

    ls_epilogue<TM, TN, WN>(p, acc, smem, wave, lane, m0, n0, wave_m0, wave_n0);
}

#ifdef DGP_DIAG
// the fp32 kernels (ls: the loader-specialised one)
static void diag_report_f32(const ConvArgs& a, int BM, int BN, bool ls, long long nwg, hipStream_t s) {
    if (!a.dbg) return;
    double v[8];
    diag_fetch(a, nwg, s, v);
    if (ls)
        printf("[diag LS %dx%d] tiles %lld nk %d | compute wave 0: first barrier %.0f cyc | per K-step: mfma+ldsread %.0f barrier-wait %.0f\n",
               BM, BN, nwg, a.nk, v[0], v[4] / a.nk, v[7] / a.nk);
    else
        printf("[diag %dx%d] tiles %lld nk %d | cycles/tile: prologue %.0f loop %.0f epilogue %.0f | per K-step (wave 0): "
               "gload-issue %.0f mfma+ldsread %.0f vmcnt-wait %.0f lds-store %.0f barrier %.0f\n", BM, BN, nwg, a.nk,
               v[0], v[1], v[2], v[3] / a.nk, v[4] / a.nk, v[5] / a.nk, v[6] / a.nk, v[7] / a.nk);
}
#endif

// The plans of the fp32 families: what the kernels refuse, the tiles and the grid
static hipError_t plan_ls(ConvArgs& a, int BM, int BN, ConvPlan& pl) {
    a.mtiles = (a.M + BM - 1) / BM;
    a.ntiles = (a.CoutP + BN - 1) / BN;
    if (a.CoutP % BN != 0 || a.Cin < 32 || a.out_mode != 0) return hipErrorInvalidValue;
    pl.grid = (long long)a.mtiles * a.ntiles;
    return hipSuccess;
}
static hipError_t plan_f32(ConvArgs& a, int BM, int BN, ConvPlan& pl) {
    a.mtiles = (a.M + BM - 1) / BM;
    a.ntiles = (a.CoutP + BN - 1) / BN;
    if (a.CoutP % BN != 0) return hipErrorInvalidValue;       // weight panels are padded to the tile
    if (a.ksplit > 1 && (a.out_mode != 1 || a.nk % a.ksplit != 0)) return hipErrorInvalidValue;
    pl.grid = (long long)a.mtiles * a.ntiles * (a.ksplit > 1 ? a.ksplit : 1);
    return hipSuccess;
}

template <int BM, int BN>
static hipError_t launch_conv_ls(const ConvArgs& a_planned, const ConvPlan& pl, hipStream_t s) {
    ConvArgs a = a_planned;
    const size_t smem = (size_t)(2 * 8 * (BM + 1) + 2 * 8 * BN) * 16;
    constexpr auto kern = conv_igemm_f32_ls<BM, BN>;
    hipError_t e = ensure_dynamic_lds<kern>(160 * 1024);
    if (e != hipSuccess) return e;
    const long long nwg = pl.grid;
#ifdef DGP_DIAG
    a.dbg = diag_buffer(nwg);
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(512), smem, s, a);
#ifdef DGP_DIAG
    diag_report_f32(a, BM, BN, true, nwg, s);
#endif
    return hipGetLastError();
}

template <int BM, int BN, int WAVES_M, int WAVES_N, bool WIDE>
static hipError_t launch_conv_t(const ConvArgs& a_planned, const ConvPlan& pl, hipStream_t s) {
    ConvArgs a = a_planned;
    const size_t smem = (size_t)(2 * 8 * (BM + 1) + 2 * 8 * BN) * 16;
    constexpr auto kern = conv_igemm_f32<BM, BN, WAVES_M, WAVES_N, WIDE>;
    hipError_t e = ensure_dynamic_lds<kern>(160 * 1024);
    if (e != hipSuccess) return e;
    const long long nwg = pl.grid;
#ifdef DGP_DIAG
    a.dbg = diag_buffer(nwg);
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64 * WAVES_M * WAVES_N), smem, s, a);
#ifdef DGP_DIAG
    diag_report_f32(a, BM, BN, false, nwg, s);
#endif
    return hipGetLastError();
}


hipError_t plan_conv_f32(ConvArgs& a, ConvPlan& pl) {
    const TileInfo& t = TILES[pl.tile];
    return pl.family == FAM_LS ? plan_ls(a, t.BM, t.BN, pl) : plan_f32(a, t.BM, t.BN, pl);
}

hipError_t launch_conv_f32(const ConvArgs& a, const ConvPlan& pl, hipStream_t s) {
    if (!pl.wide) {      // the per-lane tap kernels of Cin < 32 (plan_conv leaves one of three tiles)
        if (pl.tile == TILE_128x32) return launch_conv_t<128, 32, 4, 1, false>(a, pl, s);
        if (pl.tile == TILE_128x128) return launch_conv_t<128, 128, 2, 2, false>(a, pl, s);
        return launch_conv_t<128, 64, 2, 2, false>(a, pl, s);
    }
    return for_tile(pl.tile, [&](auto id) {
        constexpr TileInfo t = TILES[decltype(id)::value];
        if constexpr (t.family == FAM_LS) return launch_conv_ls<t.BM, t.BN>(a, pl, s);
        else if constexpr (t.family == FAM_F32) return launch_conv_t<t.BM, t.BN, t.WM, t.WN, true>(a, pl, s);
        else return hipErrorInvalidValue;
    });
}

}  // namespace dgp
