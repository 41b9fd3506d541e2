// What the conv kernel sources share (dgp_conv_f32.hip, dgp_conv_split.hip) and what the launch layer (dgp_kernels.hip) needs of
// them: the epilogues both families inline, the diagnostic build's stamp buffer, the TILES table and each family's two entries.
// Not part of the ABI.
#pragma once
#include "dgp_internal.h"
#include "dgp_device.h"
#include <utility>
#include <vector>

namespace dgp {

#ifdef DGP_DIAG
// diagnostic build only (scripts/diag.sh): s_memtime stamps fence the schedule; read SHARES, not totals
#define DIAG_STAMP(x)                                                                   \
    do {                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                              \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(x)::"memory");       \
        __builtin_amdgcn_sched_barrier(0);                                              \
    } while (0)
#else
#define DIAG_STAMP(x)
#endif

typedef float floatx16 __attribute__((ext_vector_type(16)));

// Epilogue of the loader-specialised kernels (compute waves only; wave-private LDS staging, no workgroup
// barriers: the loader waves are gone).  acc -> scale/bias/residual/ReLU/mask -> 16-byte stores.
// M16: the caller's accumulators are the 2 x 8 blocks of v_mfma_f32_16x16x32 and it has staged them into the wave's LDS tile itself
// (block (i, j) register r of lane l = row 16 i + 4 (l >> 4) + r, column 16 j + (l & 15)); `acc` is not read
template <int TM, int TN, int WN, bool M16 = false>
__device__ __forceinline__ void ls_epilogue(const ConvArgs& p, floatx16 (&acc)[TM][TN], char* smem, int wave, int lane,
                                            int m0, int n0, int wave_m0, int wave_n0, float post = 1.f) {
    constexpr int LDC = WN + 4;
    const int half = lane >> 5, l31 = lane & 31;
    const int HoWo = p.Ho * p.Wo;
    float* sC = reinterpret_cast<float*>(smem) + wave * ((M16 ? 32 * TM : 32) * LDC);      // (M16: the caller staged all 32 TM rows)
    // the wave's range slot, read NOW (see ls_epilogue_h2: nothing may wait at the end of the wave)
    unsigned slot_bits = 0u;
    if (p.out_absmax)
        slot_bits = __hip_atomic_load(reinterpret_cast<const unsigned*>(p.out_absmax) + ((int)(blockIdx.x * 8u + (threadIdx.x >> 6)) & (ABSMAX_SLOTS - 1)),
                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    constexpr int C4 = WN / 4;
    constexpr int NV = 32 * C4 / 64;
    const __amdgpu_buffer_rsrc_t rs_res =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res ? p.res : p.in), 0, p.res ? (int)p.res_bytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)p.out_bytes, 0x00020000);
    // fp16 high / low copy of the output (ConvArgs::shadow): this lane's 4 channels are half of an 8-channel cell
    const float sh_scale = p.shadow ? shadow_scale_for(p.shadow_prev, lane) : 0.f;
    const __amdgpu_buffer_rsrc_t rs_sh =
        __builtin_amdgcn_make_buffer_rsrc(p.shadow ? p.shadow : p.out, 0, sh_scale > 0.f ? (int)(p.shadow_fmt == 2 ? p.out_bytes >> 1 : p.out_bytes) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_mask =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.mask ? p.mask : p.in), 0, p.mask ? (int)p.out_bytes : 0, 0x00020000);
    const int my_c4 = lane % C4;
    const int my_r0 = lane / C4;
    const int co4 = n0 + wave_n0 + 4 * my_c4;
    const bool cok = co4 < p.Cout;
    float4 sc4 = make_float4(1.f, 1.f, 1.f, 1.f), bi4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok && p.scale) sc4 = *reinterpret_cast<const float4*>(p.scale + co4);
    if (cok && p.bias) bi4 = *reinterpret_cast<const float4*>(p.bias + co4);
    sc4.x *= post; sc4.y *= post; sc4.z *= post; sc4.w *= post;       // exact: post is a power of two (1 unless fp16-split)
    float amax = 0.f;
    // Rows go out in chunks of VC (register pressure: 8 rows of residual + gate next to the accumulators spilled them) and the
    // chunks are software-pipelined: the residual / gate loads of chunk q + 1 are in flight while chunk q is combined and stored,
    // so a wave pays one HBM round trip per tile instead of one per chunk.  The loads exist only when the layer has them.
    constexpr int VC = NV > 2 ? 2 : NV;
    constexpr int CPP = NV / VC;                   // chunks per pass (pass = one 32-row block of the wave tile)
    constexpr int NQ = TM * CPP;
    unsigned ooff[2][VC];
    float4 rres[2][VC];
    auto issue = [&](int q, int slot) {
        const int i = q / CPP, v0 = (q % CPP) * VC;
#pragma unroll
        for (int u = 0; u < VC; ++u) {
            const int row = my_r0 + (v0 + u) * (64 / C4);
            const int m = m0 + wave_m0 + 32 * i + row;
            const bool ok = cok && m < p.M;
            ooff[slot][u] = ok ? ((unsigned)(m * p.Cout + co4) << 2) : OOB;
            rres[slot][u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.res) {
                unsigned roff = OOB;
                if (p.res_s == 1) {
                    roff = ooff[slot][u];
                } else if (p.res_s == -2 && ok) {
                    const int n = m / HoWo, rem = m - n * HoWo, ho = rem / p.Wo, wo = rem - ho * p.Wo;
                    if (!((ho | wo) & 1)) roff = (unsigned)(((n * p.res_H + (ho >> 1)) * p.res_W + (wo >> 1)) * p.Cout + co4) << 2;
                } else if (p.res_s > 1 && ok) {
                    const int n = m / HoWo, rem = m - n * HoWo, ho = rem / p.Wo, wo = rem - ho * p.Wo;
                    roff = (unsigned)(((n * p.res_H + ho * p.res_s) * p.res_W + wo * p.res_s) * p.Cout + co4) << 2;
                }
                rres[slot][u] = buf_load16(rs_res, roff);
            }
        }
    };
#ifdef DGP_DIAG
    unsigned long long g0, g1, g2, g3, g4;
    DIAG_STAMP(g0);
#endif
    issue(0, 0);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i = q / CPP, v0 = (q % CPP) * VC, slot = q & 1;
#ifdef DGP_DIAG
        if (q == 1) DIAG_STAMP(g2);
#endif
        if (q % CPP == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // own reads of the previous pass are done
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!M16) {      // (M16: the caller has staged its 16x16 blocks already)
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                        sC[row * LDC + 32 * j + l31] = acc[i][j][r];
                    }
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // a wave's LDS ops complete in order
#ifdef DGP_DIAG
            if (q == 0) DIAG_STAMP(g1);
#endif
        }
        if (q + 1 < NQ) issue(q + 1, slot ^ 1);
        float4 rmask[VC];          // ReLU gate of the training step's data-gradient convs: not pipelined (keeps the forward lean)
        if (p.mask) {
#pragma unroll
            for (int u = 0; u < VC; ++u) {
                if (p.mask_fmt == 2) {      // H1 gate tensor: this lane's 4 channels are 8 bytes at half the fp32 offset
                    const u32x2 mh = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_mask, (int)(ooff[slot][u] >> 1), 0, 0));
                    rmask[u] = h2_gate4(mh, u32x2{0u, 0u});
                } else if (p.mask_fmt) {      // H2 gate tensor: this lane's 4 channels are 8 bytes of the cell's high chunk and 8 of its low chunk
                    const unsigned mo = (ooff[slot][u] & ~31u) + ((ooff[slot][u] & 16u) >> 1);
                    // (bit_cast: the builtin's result converts to a vector by splatting its low dword)
                    const u32x2 mh = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_mask, (int)mo, 0, 0));
                    const u32x2 ml = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_mask, (int)(mo + 16u), 0, 0));
                    rmask[u] = h2_gate4(mh, ml);
                } else rmask[u] = buf_load16(rs_mask, ooff[slot][u]);
            }
        }
#pragma unroll
        for (int u = 0; u < VC; ++u) {
            const int row = my_r0 + (v0 + u) * (64 / C4);
            const float4 a = *reinterpret_cast<const float4*>(sC + ((M16 ? 32 * i : 0) + row) * LDC + 4 * my_c4);
            float4 o;
            o.x = a.x * sc4.x + bi4.x + rres[slot][u].x;
            o.y = a.y * sc4.y + bi4.y + rres[slot][u].y;
            o.z = a.z * sc4.z + bi4.z + rres[slot][u].z;
            o.w = a.w * sc4.w + bi4.w + rres[slot][u].w;
            if (p.relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
            if (p.mask) {
                o.x = rmask[u].x > 0.f ? o.x : 0.f; o.y = rmask[u].y > 0.f ? o.y : 0.f;
                o.z = rmask[u].z > 0.f ? o.z : 0.f; o.w = rmask[u].w > 0.f ? o.w : 0.f;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_out, (int)ooff[slot][u], 0, 0);
            if (sh_scale > 0.f && p.shadow_fmt == 2) {
                // H1 copy (the 16-bit trainer): this lane's 4 channels are 8 bytes of the tensor at half the fp32 offset
                uint2 sh, sl;
                split2_f16(o, sh_scale, sh, sl);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{sh.x, sh.y}, rs_sh, (int)(ooff[slot][u] >> 1), 0, 0);
            } else if (sh_scale > 0.f) {
                // this lane holds 4 of a cell's 8 channels: trade halves with the neighbour (quad_perm 1,0,3,2) so that the even lane
                // stores the whole high chunk and the odd lane the whole low chunk -- one 16-byte store per lane, whole cells per pair
                uint2 sh, sl;
                split2_f16(o, sh_scale, sh, sl);
                const bool odd = my_c4 & 1;
                const unsigned g0 = odd ? sh.x : sl.x, g1 = odd ? sh.y : sl.y;
                const unsigned r0 = (unsigned)__builtin_amdgcn_mov_dpp((int)g0, 0xB1, 0xF, 0xF, true);
                const unsigned r1 = (unsigned)__builtin_amdgcn_mov_dpp((int)g1, 0xB1, 0xF, 0xF, true);
                const u32x4 cell = odd ? u32x4{r0, r1, sl.x, sl.y} : u32x4{sh.x, sh.y, r0, r1};
                __builtin_amdgcn_raw_buffer_store_b128(cell, rs_sh, (int)((ooff[slot][u] & ~31u) + (odd ? 16u : 0u)), 0, 0);
            }
            if (ooff[slot][u] != OOB) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
        }
    }
#ifdef DGP_DIAG
    DIAG_STAMP(g3);
#endif
    if (p.out_absmax) track_absmax_known(p.out_absmax, amax, lane, (int)(blockIdx.x * 8u + (threadIdx.x >> 6)), slot_bits);
#ifdef DGP_DIAG
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DIAG_STAMP(g4);
    if (p.dbg && threadIdx.x == 0) {      // (slots 3, 5, 6 are the loader stamps of the register-staged kernels: read these with DGP_DMA=1)
        unsigned long long* d = p.dbg + 10ull * blockIdx.x;
        d[3] = g1 - g0; d[5] = g2 - g1; d[6] = g3 - g2; d[8] = g4 - g3;
    }
#endif
}

// Raw accumulators of a wave tile -> a dense [rows][ld] fp32 matrix (K-split slabs of the grid's tail): same wave-private LDS
// staging as ls_epilogue, no epilogue arithmetic.
template <int TM, int TN, int WN, bool M16 = false>
__device__ __forceinline__ void ls_store_raw(floatx16 (&acc)[TM][TN], char* smem, int wave, int lane, int wave_m0, int wave_n0,
                                             float* out, int ld) {
    constexpr int LDC = WN + 4;
    constexpr int C4 = WN / 4;
    constexpr int NV = 32 * C4 / 64;
    const int half = lane >> 5, l31 = lane & 31;
    float* sC = reinterpret_cast<float*>(smem) + wave * ((M16 ? 32 * TM : 32) * LDC);
    const int my_c4 = lane % C4, my_r0 = lane / C4;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (!M16) sC[((r & 3) + 8 * (r >> 2) + 4 * half) * LDC + 32 * j + l31] = acc[i][j][r];
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int row = my_r0 + v * (64 / C4);
            *reinterpret_cast<float4*>(out + (size_t)(wave_m0 + 32 * i + row) * ld + wave_n0 + 4 * my_c4) =
                *reinterpret_cast<const float4*>(sC + ((M16 ? 32 * i : 0) + row) * LDC + 4 * my_c4);
        }
    }
}

#ifdef DGP_DIAG
// Diagnostic build: the stamp buffer the kernels write through ConvArgs::dbg (10 counters per workgroup; behind 65536 of those, 3 timeline
// words per workgroup of the split kernels).  The reports printed after a launch (parsed by scripts/diag_net.py, launch_causes.py,
// cu_phase.py) are diag_report_f32 / diag_report_split, each beside its kernels
inline unsigned long long* diag_buffer(long long nwg) {
    static unsigned long long* buf = nullptr;
    if (!buf) (void)hipMalloc(&buf, 13 * 8 * 65536);
    return nwg <= 65536 ? buf : nullptr;
}
// waits for the launch; h: the 10 counters of every workgroup, v: the mean of the first 8
inline std::vector<unsigned long long> diag_fetch(const ConvArgs& a, long long nwg, hipStream_t s, double (&v)[8]) {
    (void)hipStreamSynchronize(s);
    std::vector<unsigned long long> h(10 * nwg);
    (void)hipMemcpy(h.data(), a.dbg, 80 * nwg, hipMemcpyDeviceToHost);
    for (int k = 0; k < 8; ++k) v[k] = 0;
    for (long long b = 0; b < nwg; ++b) for (int k = 0; k < 8; ++k) v[k] += (double)h[10 * b + k];
    for (int k = 0; k < 8; ++k) v[k] /= (double)nwg;
    return h;
}
#endif

// What every TileCfg id means, in id order: the kernel family and its template parameters, and the fp32 tiles that take the launch where
// the tile's own kernel cannot.  pick_tile's DGP_FORCE_TILE check, conv_kernel_name and launch_conv all read this table.
struct TileInfo {
    int id;
    TileFamily family;
    int BM, BN;
    int WM, WN;              // fp32 family: waves along M and N
    int NT, BK, CW;          // split family: MFMAs per product (6 / 3 bf16, 2 = three fp16), K floats per step, compute waves
    bool needs_ranges;       // needs the operand ranges (fp16 split)
    int f32_tile;            // the fp32 tile that runs out_mode != 0 (itself for the fp32 family)
    int small_tile;          // the fp32 tile whose per-lane tap kernel runs Cin < 32
    const char* name;        // conv_kernel_name (nullptr: "f32")
    const char* name_h1;     // ... of an H1 launch, where it differs
};
constexpr TileInfo TILES[] = {
    {TILE_128x128,         FAM_F32,   128, 128, 2, 2, 0, 0,  0, false, TILE_128x128,    TILE_128x128, nullptr, nullptr},
    {TILE_128x64,          FAM_F32,   128, 64,  2, 2, 0, 0,  0, false, TILE_128x64,     TILE_128x64,  nullptr, nullptr},
    {TILE_64x64,           FAM_F32,   64,  64,  2, 2, 0, 0,  0, false, TILE_64x64,      TILE_128x64,  nullptr, nullptr},
    {TILE_128x32,          FAM_F32,   128, 32,  4, 1, 0, 0,  0, false, TILE_128x32,     TILE_128x32,  nullptr, nullptr},
    {TILE_128x128_W8,      FAM_F32,   128, 128, 2, 4, 0, 0,  0, false, TILE_128x128_W8, TILE_128x128, nullptr, nullptr},
    {TILE_128x128_LS,      FAM_LS,    128, 128, 0, 0, 0, 0,  0, false, TILE_128x128_W8, TILE_128x128, nullptr, nullptr},
    {TILE_128x64_LS,       FAM_LS,    128, 64,  0, 0, 0, 0,  0, false, TILE_128x64,     TILE_128x64,  nullptr, nullptr},
    {TILE_128x128_S6,      FAM_SPLIT, 128, 128, 0, 0, 6, 32, 4, false, TILE_128x128_W8, TILE_128x128, "split6_128x128_k32", nullptr},
    {TILE_128x128_S3,      FAM_SPLIT, 128, 128, 0, 0, 3, 32, 4, false, TILE_128x128_W8, TILE_128x128, "split3_128x128_k32", nullptr},
    {TILE_128x64_S6,       FAM_SPLIT, 128, 64,  0, 0, 6, 32, 4, false, TILE_128x64,     TILE_128x64,  "split6_128x64_k32", nullptr},
    {TILE_128x128_S6K16,   FAM_SPLIT, 128, 128, 0, 0, 6, 16, 4, false, TILE_128x128_W8, TILE_128x128, "split6_128x128_k16", nullptr},
    {TILE_128x128_S3K16,   FAM_SPLIT, 128, 128, 0, 0, 3, 16, 4, false, TILE_128x128_W8, TILE_128x128, "split3_128x128_k16", nullptr},
    {TILE_128x128_S6K16W8, FAM_SPLIT, 128, 128, 0, 0, 6, 16, 8, false, TILE_128x128_W8, TILE_128x128, "split6_128x128_k16w8", nullptr},
    {TILE_128x128_H3K16,   FAM_SPLIT, 128, 128, 0, 0, 2, 16, 4, true,  TILE_128x128_W8, TILE_128x128, "splith3_128x128_k16", nullptr},
    {TILE_128x128_H3K16W8, FAM_SPLIT, 128, 128, 0, 0, 2, 16, 8, true,  TILE_128x128_W8, TILE_128x128, "splith3_128x128_k16w8", nullptr},
    {TILE_128x64_H3,       FAM_SPLIT, 128, 64,  0, 0, 2, 32, 4, true,  TILE_128x64,     TILE_128x64,  "splith3_128x64_k32", "h1_128x64_k64"},
    {TILE_128x128_H3K32,   FAM_SPLIT, 128, 128, 0, 0, 2, 32, 4, true,  TILE_128x128_W8, TILE_128x128, "splith3_128x128_k32", "h1_128x128_k64"},
};
constexpr int N_TILES = (int)(sizeof(TILES) / sizeof(TILES[0]));
constexpr bool tiles_in_id_order() { for (int i = 0; i < N_TILES; ++i) if (TILES[i].id != i) return false; return true; }
static_assert(N_TILES == TILE_128x128_H3K32 + 1 && tiles_in_id_order(), "TILES is indexed by TileCfg id");

// f(std::integral_constant<int, ID>{}) for the row ID == id of TILES: how a family source turns a run-time tile id into the template
// parameters of its kernels (each instantiates its own rows only); hipErrorInvalidValue for an id outside the table
template <class F, int... ID>
inline hipError_t for_tile(int id, F&& f, std::integer_sequence<int, ID...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)((id == ID && ((e = f(std::integral_constant<int, ID>{})), true)) || ...);
    return e;
}
template <class F>
inline hipError_t for_tile(int id, F&& f) { return for_tile(id, f, std::make_integer_sequence<int, N_TILES>{}); }

// What the families export to the launch layer: the plan and the launch of tile pl.tile (set by plan_conv, with pl.family and
// pl.wide).  The plans fill the ConvArgs fields their kernels read and pl.grid (the split family: pl.path too); no HIP calls
hipError_t plan_conv_f32(ConvArgs& a, ConvPlan& pl);                                      // FAM_F32 and FAM_LS
hipError_t launch_conv_f32(const ConvArgs& a, const ConvPlan& pl, hipStream_t s);
hipError_t plan_conv_split(ConvArgs& a, int n_cu, ConvPlan& pl);                          // FAM_SPLIT
hipError_t launch_conv_split(const ConvArgs& a, const ConvPlan& pl, hipStream_t s);

}  // namespace dgp

