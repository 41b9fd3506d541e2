// gfx950 (MI355X / CDNA4): the hot path of frame selection -- which frames of a video to label (extract_frames) and which of the
// frames a model got wrong to label next (extract_outlier_frames).  The reference decodes every candidate frame, shrinks it to a
// 30-pixel-wide thumbnail and clusters the thumbnails (deeplabcut/utils/frameselectiontools.py:139-246, "On large videos this code is
// slow"); here the frames are already on the device, the thumbnails are one pass over them and the clustering is three small kernels.
//
//   frame_features_kernel<VEC>   exact integer area averages: one workgroup per (frame, output row), per-column counters in LDS
//   kmeans_colsum / _mean / _sub DATA - DATA.mean(axis=0): double column sums over fixed slabs of rows, combined in slab order
//   kmeans_assign_kernel         nearest centre in the direct form sum (x - c)^2, fp32, a fixed summation order, centres in LDS
//   kmeans_member_sum / _finish  new centres: per-slab double sums of the members in row order, combined in slab order
//
// A selection must not change from run to run: integer atomics only (LDS counters, the `changed` counter), never a float atomic, and
// every fp32 / fp64 sum has ONE order, written down in include/dgp_hip.h so that the host executor (frame_selection.py) restates it bit
// for bit.  Every product and sum rounds on its own: contraction is off for the whole file.
#include "dgp_engine.h"

#include <string>

#pragma clang fp contract(off)

namespace dgp {

// ------------------------------------------------------------------------------------------------
// Thumbnails.  HBM-bound: algorithmic bytes = the window's rows, read once.
// A work item is (row group g, unit u): unit u is the VEC bytes [u VEC, u VEC + VEC) of a frame row -- the same columns in every row,
// since a row starts VEC-aligned by the host's choice of VEC -- and the item adds them over the rows y0 + g, y0 + g + G, ... of the box
// in 16-bit lanes (at most FEAT_ROWS rows between flushes: 255 x 256 < 2^16), then hands each byte's sum to its column's counter.
// ------------------------------------------------------------------------------------------------
constexpr int FEAT_THREADS = 256;
constexpr int FEAT_MAX_WC = 16384;      // colbin: one uint16 per window column (32 KB of LDS)
constexpr int FEAT_MAX_OW = 1024;       // counters: 3 x ow uint32 (12 KB)
constexpr int FEAT_ROWS = 256;

struct FeatArgs {
    const uint8_t* frames;
    float* out;
    long long frame_stride, out_stride;
    int W, x1, y1, Wc, Hc, ow, oh, color;
};

template <int VEC>
__global__ __launch_bounds__(FEAT_THREADS) void frame_features_kernel(const FeatArgs p) {
    __shared__ unsigned short colbin[FEAT_MAX_WC];
    __shared__ unsigned counters[3 * FEAT_MAX_OW];
    const int tid = threadIdx.x;
    const long long f = blockIdx.x / (unsigned)p.oh;
    const int r = blockIdx.x % (unsigned)p.oh;
    const int nc = p.color ? 3 * p.ow : p.ow;
    for (int i = tid; i < nc; i += FEAT_THREADS) counters[i] = 0u;
    // column c lies in box i = floor(((c + 1) ow - 1) / Wc): the largest i with floor(i Wc / ow) <= c
    for (int c = tid; c < p.Wc; c += FEAT_THREADS) colbin[c] = (unsigned short)((((long long)c + 1) * p.ow - 1) / p.Wc);
    __syncthreads();
    const int ya = p.y1 + (int)(((long long)r * p.Hc) / p.oh), yb = p.y1 + (int)(((long long)(r + 1) * p.Hc) / p.oh);
    const int xb0 = p.x1 * 3, xb1 = xb0 + p.Wc * 3;               // the window's bytes inside a frame row
    const int u0 = xb0 / VEC, nu = (xb1 - 1) / VEC - u0 + 1;
    const int rows = yb - ya;
    int G = FEAT_THREADS / nu;
    G = G < 1 ? 1 : (G > rows ? rows : G);
    const uint8_t* frame = p.frames + f * p.frame_stride;
    const long long pitch = (long long)p.W * 3;
    constexpr int NW = VEC == 16 ? 4 : 1;                          // 32-bit words of a unit
    for (int item = tid; item < G * nu; item += FEAT_THREADS) {
        const int g = item / nu, u = u0 + item % nu;
        for (int yc = ya + g; yc < yb; yc += G * FEAT_ROWS) {
            const int yend = min(yb, yc + G * FEAT_ROWS);
            unsigned even[NW], odd[NW];                            // bytes 0, 2 and 1, 3 of each word, two 16-bit sums per register
#pragma unroll
            for (int w = 0; w < NW; ++w) even[w] = odd[w] = 0u;
#pragma unroll 4
            for (int y = yc; y < yend; y += G) {
                const uint8_t* src = frame + y * pitch + (long long)u * VEC;
                unsigned v[NW];
                if (VEC == 16) {
                    const uint4 q = *reinterpret_cast<const uint4*>(src);
                    v[0] = q.x; v[NW > 1 ? 1 : 0] = q.y; v[NW > 1 ? 2 : 0] = q.z; v[NW > 1 ? 3 : 0] = q.w;
                } else if (VEC == 4) {
                    v[0] = *reinterpret_cast<const unsigned*>(src);
                } else {
                    v[0] = *src;
                }
#pragma unroll
                for (int w = 0; w < NW; ++w) { even[w] += v[w] & 0x00FF00FFu; odd[w] += (v[w] >> 8) & 0x00FF00FFu; }
            }
            // bytes of one unit are neighbours in the row: runs of one counter are added up before they reach LDS
            int run = -1;
            unsigned acc = 0u;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int b = u * VEC + j;
                if (b < xb0 || b >= xb1) continue;
                const unsigned half = (j & 1) ? odd[j >> 2] : even[j >> 2];
                const unsigned s = (j & 2) ? half >> 16 : half & 0xFFFFu;
                const int rel = b - xb0, col = rel / 3;
                const int slot = p.color ? (rel - 3 * col) * p.ow + colbin[col] : colbin[col];
                if (slot != run) {
                    if (run >= 0 && acc) atomicAdd(&counters[run], acc);
                    run = slot; acc = 0u;
                }
                acc += s;
            }
            if (run >= 0 && acc) atomicAdd(&counters[run], acc);
        }
    }
    __syncthreads();
    float* out = p.out + f * p.out_stride + (long long)r * nc;
    for (int i = tid; i < nc; i += FEAT_THREADS) {
        const int box = i % p.ow;
        const int bw = (int)(((long long)(box + 1) * p.Wc) / p.ow) - (int)(((long long)box * p.Wc) / p.ow);
        const double count = (double)bw * (double)rows * (p.color ? 1.0 : 3.0);
        out[i] = (float)((double)counters[i] / count);
    }
}

static int round_half_even_div(long long a, long long b) {      // a / b rounded half to even, a >= 0, b > 0
    const long long q = a / b, rem = a % b;
    if (2 * rem > b || (2 * rem == b && (q & 1))) return (int)(q + 1);
    return (int)q;
}

// ------------------------------------------------------------------------------------------------
// k-means.  Slabs of rows (include/dgp_hip.h): S = min(64, ceil(N / 256)), ceil(N / S) rows each.
// ------------------------------------------------------------------------------------------------
constexpr int KM_THREADS = 256;
constexpr int KM_ASSIGN_ROWS = 32;                  // rows of a workgroup: 8 per wave
constexpr int KM_CENTRE_FLOATS = 10240;             // 40 KB of centres per chunk
constexpr int KM_MAX_DC = 512;                      // 8 columns per lane

static int km_slabs(long long N) {
    const long long s = (N + 255) / 256;
    return (int)(s < 1 ? 1 : (s > DGP_KMEANS_MAX_SLABS ? DGP_KMEANS_MAX_SLABS : s));
}
static int km_chunk(int k) {
    int dc = KM_CENTRE_FLOATS / k / 64 * 64;
    return dc > KM_MAX_DC ? KM_MAX_DC : dc;
}

// partial[s][d] = sum over the rows of slab s, in row order, of X[r][d]
__global__ __launch_bounds__(KM_THREADS) void kmeans_colsum_kernel(const float* __restrict__ X, long long N, int D, long long slab_rows,
                                                                   double* __restrict__ partial) {
    const int d = blockIdx.x * KM_THREADS + threadIdx.x;
    if (d >= D) return;
    const long long r0 = (long long)blockIdx.y * slab_rows, r1 = min(N, r0 + slab_rows);
    double acc = 0.0;
    for (long long r = r0; r < r1; ++r) acc += (double)X[r * D + d];
    partial[(long long)blockIdx.y * D + d] = acc;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_mean_kernel(const double* __restrict__ partial, int S, int D, long long N,
                                                                 float* __restrict__ mean) {
    const int d = blockIdx.x * KM_THREADS + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += partial[(long long)s * D + d];
    mean[d] = (float)(acc / (double)N);
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_sub_kernel(float* __restrict__ X, long long n, int D, const float* __restrict__ mean) {
    const long long step = (long long)gridDim.x * KM_THREADS;
    for (long long i = (long long)blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += step) X[i] = X[i] - mean[i % D];
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float* __restrict__ X, long long N, int D, const float* __restrict__ C,
                                                                   int k, int DC, int* __restrict__ labels, float* __restrict__ dist,
                                                                   int* __restrict__ changed) {
    __shared__ float cs[KM_CENTRE_FLOATS];                          // [k][DC], zeros past D
    __shared__ float sums[KM_ASSIGN_ROWS * DGP_KMEANS_MAX_K];       // [row of the workgroup][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * KM_ASSIGN_ROWS;
    for (int i = tid; i < KM_ASSIGN_ROWS * k; i += KM_THREADS) sums[i] = 0.0f;
    const int per_lane = DC / 64;
    for (int d0 = 0; d0 < D; d0 += DC) {
        __syncthreads();                                            // the chunk before is read out (first pass: sums are zeroed)
        for (int i = tid; i < k * DC; i += KM_THREADS) {
            const int c = i / DC, d = d0 + i % DC;
            cs[i] = d < D ? C[(long long)c * D + d] : 0.0f;
        }
        __syncthreads();
        for (int lr = wave; lr < KM_ASSIGN_ROWS; lr += KM_THREADS / 64) {
            const long long row = row0 + lr;
            if (row >= N) break;
            float x[KM_MAX_DC / 64];
#pragma unroll
            for (int j = 0; j < KM_MAX_DC / 64; ++j) {
                const int d = d0 + j * 64 + lane;
                x[j] = (j < per_lane && d < D) ? X[row * D + d] : 0.0f;
            }
            for (int c = 0; c < k; ++c) {
                const float* cc = cs + c * DC + lane;
                float part = 0.0f;
#pragma unroll
                for (int j = 0; j < KM_MAX_DC / 64; ++j) {
                    if (j < per_lane) {
                        const float diff = x[j] - cc[j * 64];
                        part = part + diff * diff;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) part = part + __shfl_xor(part, o, 64);
                if (lane == 0) sums[lr * k + c] = sums[lr * k + c] + part;      // (this wave alone touches its rows' sums)
            }
        }
    }
    __syncthreads();
    int moved = 0;
    for (int lr = wave; lr < KM_ASSIGN_ROWS; lr += KM_THREADS / 64) {
        const long long row = row0 + lr;
        if (row >= N) break;
        float bd = __builtin_inff();
        int bc = 0x7fffffff;
        for (int c = lane; c < k; c += 64) {
            const float v = sums[lr * k + c];
            if (v < bd || (v == bd && c < bc)) { bd = v; bc = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(bd, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (od < bd || (od == bd && oc < bc)) { bd = od; bc = oc; }
        }
        if (bc >= k) { bc = 0; bd = sums[lr * k]; }                 // every distance is NaN: centre 0, and the NaN is reported
        if (lane == 0) {
            if (labels[row] != bc) ++moved;
            labels[row] = bc;
            dist[row] = bd;
        }
    }
    if (lane == 0 && moved) atomicAdd(changed, moved);
}

// partial[s][c][d] = sum over the members of cluster c in slab s, in row order, of X[r][d]; pcount[s][c] = members, pcount[s][k] = labels
// outside [0, k).  grid (column chunks, k, S)
__global__ __launch_bounds__(KM_THREADS) void kmeans_member_sum_kernel(const float* __restrict__ X, long long N, int D,
                                                                       const int* __restrict__ labels, int k, long long slab_rows,
                                                                       double* __restrict__ partial, int* __restrict__ pcount) {
    __shared__ int lab[KM_THREADS];
    const int tid = threadIdx.x, d = blockIdx.x * KM_THREADS + tid, c = blockIdx.y, s = blockIdx.z;
    const long long r0 = (long long)s * slab_rows, r1 = min(N, r0 + slab_rows);
    double acc = 0.0;
    int members = 0, outside = 0;
    for (long long t0 = r0; t0 < r1; t0 += KM_THREADS) {
        __syncthreads();
        lab[tid] = t0 + tid < r1 ? labels[t0 + tid] : c + 1;       // (past the slab: some other cluster's, and counted nowhere)
        __syncthreads();
        const int n = (int)min((long long)KM_THREADS, r1 - t0);
        for (int i = 0; i < n; ++i) {
            const int l = lab[i];
            if (l == c) {
                ++members;
                if (d < D) acc += (double)X[(t0 + i) * D + d];
            } else if (l < 0 || l >= k) {
                ++outside;
            }
        }
    }
    if (d < D) partial[((long long)s * k + c) * D + d] = acc;
    if (blockIdx.x == 0 && tid == 0) {
        pcount[s * (k + 1) + c] = members;
        if (c == 0) pcount[s * (k + 1) + k] = outside;
    }
}

// grid (column chunks, k)
__global__ __launch_bounds__(KM_THREADS) void kmeans_finish_kernel(const double* __restrict__ partial, const int* __restrict__ pcount, int S,
                                                                   int D, int k, float* __restrict__ C, int* __restrict__ counts) {
    const int d = blockIdx.x * KM_THREADS + threadIdx.x, c = blockIdx.y;
    int n = 0;
    for (int s = 0; s < S; ++s) n += pcount[s * (k + 1) + c];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[c] = n;
        if (c == 0) {
            int bad = 0;
            for (int s = 0; s < S; ++s) bad += pcount[s * (k + 1) + k];
            counts[k] = bad;
        }
    }
    if (d >= D || n == 0) return;                                   // an empty cluster keeps its centre
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += partial[((long long)s * k + c) * D + d];
    C[(long long)c * D + d] = (float)(acc / (double)n);
}

static int km_check(const char* who, long long N, int D, int k, bool with_k) {
    const std::string w(who);
    if (N < 1 || D < 1) return fail(DGP_ERR_INVALID, w + ": N and D must be positive");
    if (D > DGP_KMEANS_MAX_D) return fail(DGP_ERR_INVALID, w + ": D = " + std::to_string(D) + " is above the limit of " + std::to_string((int)DGP_KMEANS_MAX_D));
    if (N * (long long)D >= (1LL << 31)) return fail(DGP_ERR_INVALID, w + ": N x D = " + std::to_string(N * (long long)D) + " must stay below 2^31");
    if (with_k && (k < 1 || k > DGP_KMEANS_MAX_K))
        return fail(DGP_ERR_INVALID, w + ": k = " + std::to_string(k) + " is outside 1 .. " + std::to_string((int)DGP_KMEANS_MAX_K));
    return DGP_OK;
}

static size_t km_partial_bytes(long long N, int D, int k) {      // doubles first, then (update only) the int counts
    const size_t S = (size_t)km_slabs(N);
    if (k == 0) return S * D * sizeof(double);
    return S * k * D * sizeof(double) + S * (k + 1) * sizeof(int);
}

}  // namespace dgp

using namespace dgp;

extern "C" int dgp_frame_features_u8(const uint8_t* frames, int32_t N, int32_t H, int32_t W, int64_t frame_stride, int32_t x1, int32_t x2,
                                     int32_t y1, int32_t y2, int32_t ow, int32_t oh, int32_t color, float* out, int64_t out_stride,
                                     void* stream) {
    const std::string w = "dgp_frame_features_u8: ";
    if (N < 0) return fail(DGP_ERR_INVALID, w + "negative frame count");
    if (H < 1 || W < 1 || (long long)H * W * 3 > 0x7fffffffLL) return fail(DGP_ERR_INVALID, w + "a frame must be non-empty and below 2 GiB");
    if (x1 < 0 || x2 > W || x1 >= x2 || y1 < 0 || y2 > H || y1 >= y2)
        return fail(DGP_ERR_INVALID, w + "the window x " + std::to_string(x1) + ":" + std::to_string(x2) + ", y " + std::to_string(y1) + ":" +
                                         std::to_string(y2) + " is empty or leaves the " + std::to_string(W) + " x " + std::to_string(H) + " frame");
    const int Wc = x2 - x1, Hc = y2 - y1;
    if (ow < 1) return fail(DGP_ERR_INVALID, w + "the thumbnail width must be positive");
    if (ow > Wc) return fail(DGP_ERR_INVALID, w + "a thumbnail " + std::to_string(ow) + " wide of a window " + std::to_string(Wc) +
                                                  " wide actually upsamples");
    if (Wc > FEAT_MAX_WC) return fail(DGP_ERR_INVALID, w + "the window is " + std::to_string(Wc) + " wide, the limit is " + std::to_string(FEAT_MAX_WC));
    if (ow > FEAT_MAX_OW) return fail(DGP_ERR_INVALID, w + "the thumbnail is " + std::to_string(ow) + " wide, the limit is " + std::to_string(FEAT_MAX_OW));
    int want = round_half_even_div((long long)Hc * ow, Wc);
    if (want < 1) want = 1;
    if (oh != want) return fail(DGP_ERR_INVALID, w + "oh = " + std::to_string(oh) + ", the rule gives " + std::to_string(want));
    if (oh > Hc) return fail(DGP_ERR_INVALID, w + "a thumbnail " + std::to_string(oh) + " high of a window " + std::to_string(Hc) + " high actually upsamples");
    const long long box = (long long)((Wc + ow - 1) / ow) * ((Hc + oh - 1) / oh);
    if (box * 765 > 0xFFFFFFFFLL)
        return fail(DGP_ERR_INVALID, w + "a box of " + std::to_string(box) + " pixels could overflow its 32-bit counter (limit 5614429 pixels)");
    const long long D = (long long)oh * ow * (color ? 3 : 1);
    if (N == 0) return DGP_OK;
    if (!frames || !out) return fail(DGP_ERR_INVALID, w + "null frames or output");
    if (frame_stride < (long long)H * W * 3 || out_stride < D) return fail(DGP_ERR_INVALID, w + "a stride is shorter than what it strides over");
    if ((long long)N * oh > 0x7fffffffLL) return fail(DGP_ERR_INVALID, w + "N x oh must stay below 2^31");
    FeatArgs a{};
    a.frames = frames; a.out = out; a.frame_stride = frame_stride; a.out_stride = out_stride;
    a.W = W; a.x1 = x1; a.y1 = y1; a.Wc = Wc; a.Hc = Hc; a.ow = ow; a.oh = oh; a.color = color ? 1 : 0;
    const unsigned long long align = (unsigned long long)(uintptr_t)frames | (unsigned long long)frame_stride | (unsigned long long)W * 3ULL;
    const dim3 grid((unsigned)((long long)N * oh)), block(FEAT_THREADS);
    if ((align & 15) == 0) hipLaunchKernelGGL(frame_features_kernel<16>, grid, block, 0, (hipStream_t)stream, a);
    else if ((align & 3) == 0) hipLaunchKernelGGL(frame_features_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(frame_features_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, w + hipGetErrorString(e));
    return DGP_OK;
}

extern "C" size_t dgp_kmeans_scratch_bytes(int64_t N, int32_t D, int32_t k) {
    if (N < 1 || D < 1 || D > DGP_KMEANS_MAX_D || N * (long long)D >= (1LL << 31) || k < 0 || k > DGP_KMEANS_MAX_K) return 0;
    return km_partial_bytes(N, D, k);
}

extern "C" int dgp_kmeans_center(float* X, int64_t N, int32_t D, float* mean, void* scratch, size_t scratch_bytes, void* stream) {
    if (int rc = km_check("dgp_kmeans_center", N, D, 0, false)) return rc;
    if (!X || !mean || !scratch) return fail(DGP_ERR_INVALID, "dgp_kmeans_center: null pointer");
    if (scratch_bytes < km_partial_bytes(N, D, 0) || ((uintptr_t)scratch & 7)) return fail(DGP_ERR_INVALID, "dgp_kmeans_center: scratch is too small or not 8-byte aligned");
    const int S = km_slabs(N);
    const long long slab_rows = (N + S - 1) / S;
    const unsigned cols = (unsigned)((D + KM_THREADS - 1) / KM_THREADS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_colsum_kernel, dim3(cols, (unsigned)S), dim3(KM_THREADS), 0, s, X, (long long)N, D, slab_rows, (double*)scratch);
    hipLaunchKernelGGL(kmeans_mean_kernel, dim3(cols), dim3(KM_THREADS), 0, s, (const double*)scratch, S, D, (long long)N, mean);
    const long long n = (long long)N * D;
    long long blocks = (n + KM_THREADS - 1) / KM_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kmeans_sub_kernel, dim3((unsigned)blocks), dim3(KM_THREADS), 0, s, X, n, D, (const float*)mean);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_kmeans_center: ") + hipGetErrorString(e));
    return DGP_OK;
}

extern "C" int dgp_kmeans_assign(const float* X, int64_t N, int32_t D, const float* C, int32_t k, int32_t* labels, float* dist,
                                 int32_t* changed, void* stream) {
    if (int rc = km_check("dgp_kmeans_assign", N, D, k, true)) return rc;
    if (!X || !C || !labels || !dist || !changed) return fail(DGP_ERR_INVALID, "dgp_kmeans_assign: null pointer");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(changed, 0, sizeof(int32_t), s));
    const long long blocks = (N + KM_ASSIGN_ROWS - 1) / KM_ASSIGN_ROWS;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)blocks), dim3(KM_THREADS), 0, s, X, (long long)N, D, C, k, km_chunk(k), labels, dist,
                       changed);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_kmeans_assign: ") + hipGetErrorString(e));
    return DGP_OK;
}

extern "C" int dgp_kmeans_update(const float* X, int64_t N, int32_t D, const int32_t* labels, float* C, int32_t k, int32_t* counts,
                                 void* scratch, size_t scratch_bytes, void* stream) {
    if (int rc = km_check("dgp_kmeans_update", N, D, k, true)) return rc;
    if (!X || !labels || !C || !counts || !scratch) return fail(DGP_ERR_INVALID, "dgp_kmeans_update: null pointer");
    if (scratch_bytes < km_partial_bytes(N, D, k) || ((uintptr_t)scratch & 7)) return fail(DGP_ERR_INVALID, "dgp_kmeans_update: scratch is too small or not 8-byte aligned");
    const int S = km_slabs(N);
    const long long slab_rows = (N + S - 1) / S;
    const unsigned cols = (unsigned)((D + KM_THREADS - 1) / KM_THREADS);
    double* partial = (double*)scratch;
    int* pcount = (int*)(partial + (size_t)S * k * D);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_member_sum_kernel, dim3(cols, (unsigned)k, (unsigned)S), dim3(KM_THREADS), 0, s, X, (long long)N, D, labels, k, slab_rows,
                       partial, pcount);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(cols, (unsigned)k), dim3(KM_THREADS), 0, s, (const double*)partial, (const int*)pcount, S, D, k, C,
                       counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_kmeans_update: ") + hipGetErrorString(e));
    return DGP_OK;
}
