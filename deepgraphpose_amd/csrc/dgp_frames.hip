// gfx950 (MI355X / CDNA4): a training batch of the DGP drivers assembled on the device from frames that are already there.  The
// reference reads every frame of every batch from the video (Dataset.load_data, DGP/dataset.py:811-821) and feeds the stack
// (fitdgp.py:762-764); here the run's selected frames are decoded once into a store of equal-pitch slots, and a batch is one launch
// that copies nt of them -- or frames of a small `patch` uploaded for this iteration -- into a contiguous [nt][H][W][3] block.
//
// gather_frames_kernel<V>: blockIdx.y is the output frame, its source comes from a table of at most GATHER_FRAMES entries that
// travels in the launch arguments (no copy of its own, nothing to keep alive); blockIdx.x strides over the frame in units of V =
// uint4 (16 bytes, four in flight per thread) or V = uint8_t.  A pure copy: plain vector loads and stores, no LDS, no atomics.  The
// host picks the 16-byte form only when every address it produces is 16-byte aligned (the slot pitch always is; the packed out and
// patch frames are when frame_bytes is); anything else takes the byte form.  Slot offsets are 64-bit: a store may pass 4 GiB.
#include "dgp_engine.h"

#include <string>

namespace dgp {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_FRAMES = 64;       // table entries per launch (a DGP batch has batch_size + 1 = 11 frames)
constexpr int GATHER_UNROLL = 4;
constexpr int GATHER_BLOCKS = 2048;     // blocks per launch, about: 8 per CU

struct GatherArgs {
    const uint8_t* store;
    const uint8_t* patch;
    uint8_t* out;                       // the first frame of THIS launch
    long long slot_stride, frame_bytes;
    long long units;                    // frame_bytes / sizeof(V)
    int32_t src[GATHER_FRAMES];
};

template <typename V>
__global__ __launch_bounds__(GATHER_THREADS) void gather_frames_kernel(const GatherArgs p) {
    const int f = blockIdx.y;
    const int s = p.src[f];
    const uint8_t* from = s >= 0 ? p.store + (long long)s * p.slot_stride : p.patch + (long long)(-1 - s) * p.frame_bytes;
    const V* in = reinterpret_cast<const V*>(from);
    V* out = reinterpret_cast<V*>(p.out + (long long)f * p.frame_bytes);
    const long long step = (long long)gridDim.x * GATHER_THREADS;
    long long i = (long long)blockIdx.x * GATHER_THREADS + threadIdx.x;
    for (; i + (GATHER_UNROLL - 1) * step < p.units; i += GATHER_UNROLL * step) {
        V v[GATHER_UNROLL];
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k) v[k] = in[i + k * step];
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k) out[i + k * step] = v[k];
    }
    for (; i < p.units; i += step) out[i] = in[i];
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace dgp

using namespace dgp;

extern "C" int dgp_gather_frames_u8(const uint8_t* store, int64_t n_slots, int64_t slot_stride, const uint8_t* patch, int32_t m,
                                    const int32_t* h_src, int32_t nt, int64_t frame_bytes, uint8_t* out, void* stream) {
    if (nt < 0 || n_slots < 0 || m < 0) return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: negative count");
    if (nt == 0) return DGP_OK;
    if (frame_bytes <= 0) return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: frame_bytes must be positive");
    if (!h_src || !out) return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: null table or output");
    if (n_slots > 0x7fffffffLL) return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: more than 2^31 - 1 slots");
    if (n_slots > 0 && (!store || slot_stride % 16 != 0 || slot_stride < frame_bytes))
        return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: a store needs a pitch that is a multiple of 16 and at least frame_bytes");
    if (m > 0 && !patch) return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: null patch");
    for (int f = 0; f < nt; ++f)
        if (h_src[f] >= n_slots || h_src[f] < -(int64_t)m)
            return fail(DGP_ERR_INVALID, "dgp_gather_frames_u8: src[" + std::to_string(f) + "] = " + std::to_string(h_src[f]) +
                                             " is outside the " + std::to_string(n_slots) + " slots and the " + std::to_string(m) +
                                             " patch frames");
    const bool wide = frame_bytes % 16 == 0 && aligned16(out) && (n_slots == 0 || aligned16(store)) && (m == 0 || aligned16(patch));
    const long long units = wide ? frame_bytes / 16 : frame_bytes;
    for (int f0 = 0; f0 < nt; f0 += GATHER_FRAMES) {
        const int nf = nt - f0 < GATHER_FRAMES ? nt - f0 : GATHER_FRAMES;
        GatherArgs a{};
        a.store = store; a.patch = patch;
        a.out = out + (long long)f0 * frame_bytes;
        a.slot_stride = slot_stride; a.frame_bytes = frame_bytes; a.units = units;
        for (int f = 0; f < nf; ++f) a.src[f] = h_src[f0 + f];
        const long long per_block = (long long)GATHER_THREADS * GATHER_UNROLL;
        long long bx = (units + per_block - 1) / per_block;
        const long long cap = (GATHER_BLOCKS + nf - 1) / nf;
        if (bx > cap) bx = cap;
        const dim3 grid((unsigned)bx, (unsigned)nf);
        if (wide)
            hipLaunchKernelGGL(gather_frames_kernel<uint4>, grid, dim3(GATHER_THREADS), 0, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL(gather_frames_kernel<uint8_t>, grid, dim3(GATHER_THREADS), 0, (hipStream_t)stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_gather_frames_u8: ") + hipGetErrorString(e));
    }
    return DGP_OK;
}
