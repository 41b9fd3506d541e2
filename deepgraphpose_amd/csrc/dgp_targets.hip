// gfx950 (MI355X / CDNA4): DLC's target maps (compute_target_part_scoremap, PET/dataset/pose_defaultdataset.py:220-266) for a batch of
// frames, built on the device from a handful of (joint, x, y) entries instead of on the host as four mostly-zero [n, H, W, *] arrays
// that are then uploaded.  The values are the host function's float64 results cast to fp32, bit for bit: every product and sum
// below rounds on its own (contraction off), the quotient is an IEEE division and rint is Python's half-even round.
//
// target_maps_kernel<JPT>: a thread owns one cell (frame, y, x) and JPT consecutive joints of it, and writes ALL of their outputs --
// zeros included, so no output is cleared first.  It walks the frame's entries in order; an entry of one of its joints whose window
// holds the cell and whose disk holds the cell's centre sets that joint's values, a later one overwrites them (the host loop's
// order).  JPT = 4 when nj is a multiple of 4: scmap / weights leave as one 16-byte store, lmap / lmask as two; otherwise JPT = 1 with
// a 4-byte and an 8-byte store.  Threads are numbered (cell, joint group) with the group fastest: a wave's stores are contiguous.
#include "dgp_engine.h"

#include <cmath>
#include <string>

namespace dgp {

constexpr int TGT_THREADS = 256;

struct TargetArgs {
    const double* entries;              // [n_entries][3] = (joint id, x, y)
    const int32_t* offsets;             // [n + 1]
    float *scmap, *weights, *lmap, *lmask;
    int n, H, W, nj;
    int present_only;                   // weigh_only_present_joints
    double stride, half, thr, thr_sq, inv_stdev;
    long long total;                    // n * H * W * (nj / JPT) threads
};

#pragma clang fp contract(off)
template <int JPT>
__global__ __launch_bounds__(TGT_THREADS) void target_maps_kernel(const TargetArgs p) {
#pragma clang fp contract(off)
    const long long tid = (long long)blockIdx.x * TGT_THREADS + threadIdx.x;
    if (tid >= p.total) return;
    const int groups = p.nj / JPT;
    const int g = (int)(tid % groups);
    const long long cell = tid / groups;                    // (f * H + y) * W + x
    const int x = (int)(cell % p.W);
    const int y = (int)((cell / p.W) % p.H);
    const int f = (int)(cell / ((long long)p.W * p.H));
    const int j0 = g * JPT;

    float sc[JPT], pres[JPT], lx[JPT], ly[JPT];
#pragma unroll
    for (int q = 0; q < JPT; ++q) sc[q] = pres[q] = lx[q] = ly[q] = 0.0f;

    const int e1 = p.offsets[f + 1];
    for (int e = p.offsets[f]; e < e1; ++e) {
        const int q = (int)p.entries[3 * (size_t)e] - j0;
        if (q < 0 || q >= JPT) continue;
        const double jx = p.entries[3 * (size_t)e + 1], jy = p.entries[3 * (size_t)e + 2];
        // the window, as the host computes it: int cx, then float bounds clamped and rounded half-even
        const double cx = rint((jx - p.half) / p.stride), cy = rint((jy - p.half) / p.stride);
        const double wx0 = rint(fmax(cx - p.thr - 1.0, 0.0)), wx1 = rint(fmin(cx + p.thr + 1.0, (double)(p.W - 1)));
        const double wy0 = rint(fmax(cy - p.thr - 1.0, 0.0)), wy1 = rint(fmin(cy + p.thr + 1.0, (double)(p.H - 1)));
        const double dx = jx - ((double)x * p.stride + p.half), dy = jy - ((double)y * p.stride + p.half);
        const bool in_window = !(wx1 < wx0 || wy1 < wy0) && (double)x >= wx0 && (double)x <= wx1 && (double)y >= wy0 && (double)y <= wy1;
        const bool inside = in_window && (dx * dx + dy * dy <= p.thr_sq);
#pragma unroll
        for (int k = 0; k < JPT; ++k)                       // (a constant index: the arrays stay in registers)
            if (k == q) {
                pres[k] = 1.0f;                             // the joint is labeled in this frame, inside a window or not
                if (inside) {
                    sc[k] = 1.0f;
                    lx[k] = (float)(dx * p.inv_stdev);
                    ly[k] = (float)(dy * p.inv_stdev);
                }
            }
    }

    const size_t o1 = (size_t)cell * p.nj + j0, o2 = 2 * o1;
    if constexpr (JPT == 4) {
        if (p.scmap) *(float4*)(p.scmap + o1) = make_float4(sc[0], sc[1], sc[2], sc[3]);
        if (p.weights)
            *(float4*)(p.weights + o1) = p.present_only ? make_float4(pres[0], pres[1], pres[2], pres[3]) : make_float4(1.f, 1.f, 1.f, 1.f);
        if (p.lmap) {
            *(float4*)(p.lmap + o2) = make_float4(lx[0], ly[0], lx[1], ly[1]);
            *(float4*)(p.lmap + o2 + 4) = make_float4(lx[2], ly[2], lx[3], ly[3]);
        }
        if (p.lmask) {
            *(float4*)(p.lmask + o2) = make_float4(sc[0], sc[0], sc[1], sc[1]);
            *(float4*)(p.lmask + o2 + 4) = make_float4(sc[2], sc[2], sc[3], sc[3]);
        }
    } else {
        if (p.scmap) p.scmap[o1] = sc[0];
        if (p.weights) p.weights[o1] = p.present_only ? pres[0] : 1.0f;
        if (p.lmap) *(float2*)(p.lmap + o2) = make_float2(lx[0], ly[0]);
        if (p.lmask) *(float2*)(p.lmask + o2) = make_float2(sc[0], sc[0]);
    }
}

// thr ** 2 as CPython evaluates it: libm's pow with a run-time exponent (a constant 2.0 would be folded into thr * thr, which pow is
// not guaranteed to equal in the last bit)
static double py_square(double v) {
    volatile double two = 2.0;
    return std::pow(v, two);
}

}  // namespace dgp

using namespace dgp;

extern "C" int dgp_target_maps(const double* d_entries, const int32_t* d_offsets, const double* h_entries, const int32_t* h_offsets,
                               int32_t n_frames, int32_t H, int32_t W, int32_t nj, double stride, double pos_dist_thresh, double scale,
                               double locref_stdev, int32_t weigh_only_present_joints, float* scmap, float* weights, float* lmap,
                               float* lmask, void* stream) {
#pragma clang fp contract(off)
    if (n_frames <= 0 || H <= 0 || W <= 0 || nj <= 0) return fail(DGP_ERR_INVALID, "dgp_target_maps: sizes must be positive");
    if (!(stride > 0.0) || !(locref_stdev > 0.0) || !std::isfinite(stride) || !std::isfinite(locref_stdev) ||
        !std::isfinite(pos_dist_thresh) || !std::isfinite(scale))
        return fail(DGP_ERR_INVALID, "dgp_target_maps: stride and locref_stdev must be positive, every parameter finite");
    if (!h_offsets || !d_offsets) return fail(DGP_ERR_INVALID, "dgp_target_maps: null offsets");
    if (h_offsets[0] != 0) return fail(DGP_ERR_INVALID, "dgp_target_maps: offsets must start at 0");
    for (int f = 0; f < n_frames; ++f)
        if (h_offsets[f + 1] < h_offsets[f]) return fail(DGP_ERR_INVALID, "dgp_target_maps: offsets decrease at frame " + std::to_string(f));
    const int n_entries = h_offsets[n_frames];
    if (n_entries > 0 && (!h_entries || !d_entries)) return fail(DGP_ERR_INVALID, "dgp_target_maps: null entries");
    for (int e = 0; e < n_entries; ++e) {
        const double id = h_entries[3 * (size_t)e];
        if (!(id >= 0.0 && id < (double)nj) || id != std::floor(id))
            return fail(DGP_ERR_INVALID, "dgp_target_maps: entry " + std::to_string(e) + " has a joint id outside [0, " + std::to_string(nj) + ")");
        if (!std::isfinite(h_entries[3 * (size_t)e + 1]) || !std::isfinite(h_entries[3 * (size_t)e + 2]))
            return fail(DGP_ERR_INVALID, "dgp_target_maps: entry " + std::to_string(e) + " has a coordinate that is not finite");
    }
    const int jpt = nj % 4 == 0 ? 4 : 1;
    const long long total = (long long)n_frames * H * W * (nj / jpt);
    if ((long long)n_frames * H * W * nj * 2 > 0x7fffffffLL * 2 || (total + TGT_THREADS - 1) / TGT_THREADS > 0x7fffffffLL)
        return fail(DGP_ERR_INVALID, "dgp_target_maps: maps of more than 2^32 cells");
    if (!scmap && !weights && !lmap && !lmask) return DGP_OK;
    TargetArgs a{};
    a.entries = d_entries; a.offsets = d_offsets;
    a.scmap = scmap; a.weights = weights; a.lmap = lmap; a.lmask = lmask;
    a.n = n_frames; a.H = H; a.W = W; a.nj = nj;
    a.present_only = weigh_only_present_joints ? 1 : 0;
    a.stride = stride;
    a.half = stride / 2.0;
    a.thr = pos_dist_thresh * scale;
    a.thr_sq = py_square(a.thr);
    a.inv_stdev = 1.0 / locref_stdev;
    a.total = total;
    const dim3 grid((unsigned)((total + TGT_THREADS - 1) / TGT_THREADS));
    if (jpt == 4)
        hipLaunchKernelGGL(target_maps_kernel<4>, grid, dim3(TGT_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(target_maps_kernel<1>, grid, dim3(TGT_THREADS), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_target_maps: ") + hipGetErrorString(e));
    return DGP_OK;
}
