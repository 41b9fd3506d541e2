// Training step of the DGP hot path on gfx950: forward with retained activations, backward through the
// heads / ResNet (data gradients through the same implicit-GEMM kernel, weight gradients through an
// fp32-MFMA reduction-over-pixels GEMM), BN-affine / bias gradients, global-norm clip + momentum SGD.
//
// Reference: sess.run([loss, train_op]) in fit_dgp (DGP/models/fitdgp.py:708-713,818): TF autodiff of
// dgp_loss w.r.t. ALL trainable variables (conv weights, BN gamma/beta -- moving statistics stay frozen because
// the net is built with is_training=False, PET/nnet/pose_net.py:52 -- head weights/biases),
// clip_by_global_norm(10), MomentumOptimizer(0.9).
//
// This file: the trainer (create / destroy / info / workspace plan), the forward and the backward pass with the element-wise kernels they
// launch, gradient groups, tier / fast-mode entry points.  Beside it (dgp_train.h): dgp_wgrad.hip (weight-gradient kernels),
// dgp_train_pack.hip (re-packing, weight sync), dgp_optim.hip (optimisers, step status), dgp_train_layers.hip (layer-level entry points).
#include "dgp_train.h"
#include "dgp_device.h"
#include <cstdlib>
#include <cstring>

using namespace dgp;

namespace {

// fp32 [n][C] -> fp16 high / low cells with the scale shadow_scale_for predicts from `prev` (layer-level entry point only: inside the
// training step the producers' epilogues write the copies)
__global__ __launch_bounds__(256) void f32_to_shadow_kernel(const float4* __restrict__ x, long long n8, const float* __restrict__ prev,
                                                            uint4* __restrict__ out) {
    const float s = shadow_scale_for(prev, threadIdx.x & 63);
    if (!(s > 0.f)) return;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n8; g += (long long)gridDim.x * 256) {
        const float4 a = x[2 * g], b = x[2 * g + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint4 hi, lo;
        h2_pack8(v, s, hi, lo);
        out[2 * g] = hi; out[2 * g + 1] = lo;
    }
}

// H2 tensors with predicted scales (ConvArgs::*_scale_dev): after the pass, every such tensor's measured range must lie inside the
// window its predicted scale covers, else flag |= 1 and the host repeats the step on fp32 tensors.  One wave per listed slot.
struct H2CheckList { int n; short idx[254]; };
__global__ __launch_bounds__(64) void h2_pred_check_kernel(const H2CheckList list, const float* __restrict__ pool,
                                                           const float* __restrict__ prev, int* __restrict__ flag) {
    const int k = blockIdx.x;
    if (k >= list.n) return;
    const int lane = threadIdx.x;
    const float* pv = prev + (size_t)list.idx[k] * ABSMAX_SLOTS;
    const float* cu = pool + (size_t)list.idx[k] * ABSMAX_SLOTS;
    // (bits 8..: slot + 1 of a failed tensor -- diagnostics; any non-zero value means "repeat the step")
    if (!shadow_usable(shadow_scale_for(pv, lane), cu, lane) && lane == 0) atomicOr(flag, 1 | ((list.idx[k] + 1) << 8));
}

// H2 cells with a predicted scale -> fp32 (the heads' weight gradient and gate read the block4 features as fp32)
__global__ __launch_bounds__(256) void h2_to_f32_pred_kernel(const uint4* __restrict__ x, long long n8, const float* __restrict__ prev,
                                                             float4* __restrict__ out) {
    const float s = shadow_scale_for(prev, threadIdx.x & 63);
    const float inv = s > 0.f ? 1.f / s : 0.f;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n8; g += (long long)gridDim.x * 256) {
        float v[8];
        h2_unpack8(x[2 * g], x[2 * g + 1], inv, v);
        out[2 * g] = make_float4(v[0], v[1], v[2], v[3]);
        out[2 * g + 1] = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// 16-bit tier: H1 cells with a predicted scale -> fp32 (the block4 features for the heads' backward; the data gradient that leaves the
// H1 units for block1).  gate != nullptr: an H1 tensor of the same shape, the output is zeroed where its half is not positive.
__global__ __launch_bounds__(256) void h1_to_f32_pred_kernel(const uint4* __restrict__ x, long long n8, const float* __restrict__ prev,
                                                             float4* __restrict__ out, const uint4* __restrict__ gate) {
    const float s = shadow_scale_for(prev, threadIdx.x & 63);
    const float inv = s > 0.f ? 1.f / s : 0.f;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n8; g += (long long)gridDim.x * 256) {
        float v[8];
        h1_unpack8(x[g], inv, v);
        if (gate) {
            const half8 q = __builtin_bit_cast(half8, gate[g]);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (float)q[k] > 0.f ? v[k] : 0.f;
        }
        out[2 * g] = make_float4(v[0], v[1], v[2], v[3]);
        out[2 * g + 1] = make_float4(v[4], v[5], v[6], v[7]);
    }
}
// fp32 -> H1 cells with the scale predicted from `prev` (the heads' data gradient enters the H1 units)
__global__ __launch_bounds__(256) void f32_to_h1_pred_kernel(const float4* __restrict__ x, long long n8, const float* __restrict__ prev,
                                                             uint4* __restrict__ out) {
    const float s = shadow_scale_for(prev, threadIdx.x & 63);
    if (!(s > 0.f)) return;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n8; g += (long long)gridDim.x * 256) {
        const float4 a = x[2 * g], b = x[2 * g + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        out[g] = h1_pack8(v, s);
    }
}
// zero-stuffed copy of an H1 gradient tensor [N, Ho, Wo, C] -> [N, 2 Ho, 2 Wo, C] (data at the even positions; `out` zeroed by the caller):
// the data gradient of a stride-2 conv then is a plain stride-1 conv on the cell kernels (the gather form `up = 2` has no LDS-DMA loader)
__global__ __launch_bounds__(256) void h1_zero_stuff_kernel(const uint4* __restrict__ x, int N, int Ho, int Wo, int C8, uint4* __restrict__ out) {
    const long long total = (long long)N * Ho * Wo * C8;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int c = (int)(g % C8);
        const long long px = g / C8;
        const int wo = (int)(px % Wo), ho = (int)((px / Wo) % Ho), n = (int)(px / ((long long)Wo * Ho));
        out[(((long long)n * 2 * Ho + 2 * ho) * (2 * Wo) + 2 * wo) * C8 + c] = x[g];
    }
}

// Finalisation of the parameter gradients of ALL non-head layers in two launches (blockIdx.z / .y = layer; offsets are relative to the
// workspace, which the caller may move between steps): every layer keeps its own dWraw / colsum region, so nothing has to be
// finalised between two layers' weight-gradient GEMMs.
//   scale_dw_dot_all_kernel:   dW = scale * dWraw (HWIO, real Cin) and dot[co] += sum_k W[k][co] * dWraw[k][co]
//   bn_param_grads_all_kernel: dgamma = r * (dot - mean * dbeta), dbeta = colsum           (r = rsqrt(var + eps))
struct FinDesc {
    long long dw_off, cs_off;              // bytes from the workspace base
    long long w_off, g_off, b_off, mean_off, var_off;
    int taps, cin, cin_real, cout;
    const float* d_scale;
};
__global__ __launch_bounds__(256) void scale_dw_dot_all_kernel(const FinDesc* __restrict__ table, const char* __restrict__ ws,
                                                               const float* __restrict__ params, float* __restrict__ grads,
                                                               int rows_per_block) {
    // a thread owns 4 adjacent output channels (16-byte accesses; every layer but the heads has Cout % 4 == 0 and 16-byte aligned
    // offsets) of every 16th row of the block's row range
    __shared__ float4 part[16][16];
    const FinDesc d = table[blockIdx.z];
    const int krows = d.taps * d.cin_real;
    if ((int)blockIdx.x * 64 >= d.cout || (int)blockIdx.y * rows_per_block >= krows) return;
    const float* dwraw = reinterpret_cast<const float*>(ws + d.dw_off);
    float* dot = reinterpret_cast<float*>(const_cast<char*>(ws) + d.cs_off) + d.cout;
    const float* w = params + d.w_off;
    float* dW = grads + d.w_off;
    const int c4 = threadIdx.x & 15, co = blockIdx.x * 64 + 4 * c4, rl = threadIdx.x >> 4;
    const int k0 = blockIdx.y * rows_per_block, k1 = min(krows, k0 + rows_per_block);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (co < d.cout) {
        const float4 sc = *reinterpret_cast<const float4*>(d.d_scale + co);
#pragma unroll 4
        for (int k = k0 + rl; k < k1; k += 16) {
            const int tp = k / d.cin_real, ci = k - tp * d.cin_real;
            const float4 g = *reinterpret_cast<const float4*>(dwraw + ((long long)tp * d.cin + ci) * d.cout + co);
            const long long o = (long long)k * d.cout + co;
            const float4 wv = *reinterpret_cast<const float4*>(w + o);
            acc.x += wv.x * g.x; acc.y += wv.y * g.y; acc.z += wv.z * g.z; acc.w += wv.w * g.w;
            *reinterpret_cast<float4*>(dW + o) = make_float4(sc.x * g.x, sc.y * g.y, sc.z * g.z, sc.w * g.w);
        }
    }
    part[rl][c4] = acc;
    __syncthreads();
    if (threadIdx.x < 64 && blockIdx.x * 64 + threadIdx.x < (unsigned)d.cout) {
        const int q = threadIdx.x >> 2, e = threadIdx.x & 3;
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += reinterpret_cast<const float*>(&part[r][q])[e];
        atomicAdd(dot + blockIdx.x * 64 + threadIdx.x, sum);
    }
}
__global__ void bn_param_grads_all_kernel(const FinDesc* __restrict__ table, const char* __restrict__ ws, const float* __restrict__ stats,
                                          float eps, float* __restrict__ grads) {
    const FinDesc d = table[blockIdx.y];
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= d.cout) return;
    const float* colsum = reinterpret_cast<const float*>(ws + d.cs_off);
    const float r = 1.f / sqrtf(stats[d.var_off + co] + eps);
    const float db = colsum[co];
    grads[d.b_off + co] = db;
    grads[d.g_off + co] = r * (colsum[d.cout + co] - stats[d.mean_off + co] * db);
}

// head: dw[ka][kb][c][ci] = dW'raw[(khp,kwp)][ci][(a,b),c] (each w element appears once), db[c] = sum_phases colsum
// (cpad: columns per row of dwraw; col0: first column of this head -- the 16-bit tier's merged launch holds both heads side by side)
__global__ void finalize_head_grads(const float* __restrict__ dwraw, const float* __restrict__ colsum, int njt, int cin,
                                    int cpad, int col0, float* __restrict__ dw, float* __restrict__ db) {
    const long long total = 9ll * njt * cin;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(g % cin);
        long long r = g / cin;
        const int c = (int)(r % njt);
        r /= njt;
        const int kb = (int)(r % 3), ka = (int)(r / 3);
        // ka = a + 2 - 2 khp  ->  (ka=0: a=0,khp=1) (ka=1: a=1,khp=1) (ka=2: a=0,khp=0)
        const int a = ka == 1 ? 1 : 0, khp = ka == 2 ? 0 : 1;
        const int b = kb == 1 ? 1 : 0, kwp = kb == 2 ? 0 : 1;
        dw[g] = dwraw[(((long long)(khp * 2 + kwp)) * cin + ci) * cpad + col0 + (a * 2 + b) * njt + c];
    }
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < njt) db[c] = colsum[col0 + c] + colsum[col0 + njt + c] + colsum[col0 + 2 * njt + c] + colsum[col0 + 3 * njt + c];
}

// d scoremap [N,2h,2w,njt] -> phase-major rows [N*h*w, cpad] (inverse of the forward scatter), zero padded
// (rng: range slots that take max |value| -- one array for BOTH heads' gathers: it predicts the scale of the merged H1 tensor that
// head_gather_h1_kernel writes in the next 16-bit pass)
__global__ void head_gather_kernel(const float* __restrict__ dsc, int N, int h, int w, int njt, int cpad,
                                   float* __restrict__ out, float* __restrict__ rng) {
    const long long total = (long long)N * h * w * cpad;
    float mx = 0.f;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(g % cpad);
        long long m = g / cpad;
        float v = 0.f;
        if (co < 4 * njt) {
            const int ph = co / njt, c = co - ph * njt;
            const int j = (int)(m % w);
            m /= w;
            const int i = (int)(m % h);
            const int n = (int)(m / h);
            v = dsc[(((long long)n * 2 * h + 2 * i + (ph >> 1)) * 2 * w + 2 * j + (ph & 1)) * njt + c];
        }
        out[g] = v;
        mx = fmaxf(mx, fabsf(v));
    }
    pack_track(rng, mx);
}

// 16-bit tier: both heads' loss gradients -> ONE phase-major H1 tensor [N*h*w, CT].  Columns [0, cpad0): the part head's phases as
// head_gather_kernel lays them out, [cpad0, cpad0 + cpad1): the locref head's, zero up to CT (a multiple of 64: one K-step of the H1
// kernels).  Scale: predicted from the range the same values had one step ago (prev); this step's range goes to rng.  One data-gradient
// launch and one weight-gradient launch then serve both heads.
__global__ __launch_bounds__(256) void head_gather_h1_kernel(const float* __restrict__ dsc0, const float* __restrict__ dsc1, int N, int h, int w,
                                                             int njt0, int cpad0, int njt1, int cpad1, int CT, const float* __restrict__ prev,
                                                             uint4* __restrict__ out, float* __restrict__ rng) {
    const float scale = shadow_scale_for(prev, threadIdx.x & 63);
    const int G = CT >> 3;
    const long long total = (long long)N * h * w * G;
    float mx = 0.f;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int cg = (int)(g % G);
        long long m = g / G;
        const int j = (int)(m % w);
        m /= w;
        const int i = (int)(m % h);
        const int n = (int)(m / h);
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int co = cg * 8 + k;
            const float* dsc = dsc0;
            int njt = njt0;
            if (co >= cpad0) { co -= cpad0; dsc = dsc1; njt = njt1; if (co >= cpad1) njt = 0; }
            v[k] = 0.f;
            if (co < 4 * njt) {
                const int ph = co / njt, c = co - ph * njt;
                v[k] = dsc[(((long long)n * 2 * h + 2 * i + (ph >> 1)) * 2 * w + 2 * j + (ph & 1)) * njt + c];
            }
            mx = fmaxf(mx, fabsf(v[k]));
        }
        out[g] = h1_pack8(v, scale);
    }
    pack_track(rng, mx);
}

// max-pool 3x3/2 SAME backward fused with the stem's ReLU gate: dC1 = (C1 > 0) * sum over windows whose first
// maximum is this element of dPool.
// Training forward pool: the same maxima as maxpool3x3s2_same plus, per window and channel, the position (a * 3 + b) of its FIRST
// maximum in row-major window order -- the element TF's MaxPoolGrad routes the gradient to.
__global__ __launch_bounds__(256) void maxpool_fwd_idx_kernel(const float* __restrict__ x, int N, int H, int W, int C4, int Ho, int Wo,
                                                              int pt, int pl, float* __restrict__ y, uchar4* __restrict__ idx,
                                                              uint2* __restrict__ y_h1 = nullptr, const float* __restrict__ h1_prev = nullptr) {
    // y_h1 (16-bit tier): an H1 copy of the pool output with the scale predicted from the previous step's range of conv1's output
    const float sh1 = y_h1 ? shadow_scale_for(h1_prev, threadIdx.x & 63) : 0.f;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(g % C4);
        long long pix = g / C4;
        const int wo = (int)(pix % Wo);
        pix /= Wo;
        const int ho = (int)(pix % Ho);
        const int n = (int)(pix / Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        uchar4 k = make_uchar4(255, 255, 255, 255);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int hi = ho * 2 - pt + a;
            if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int wi = wo * 2 - pl + b;
                if ((unsigned)wi >= (unsigned)W) continue;
                const float4 v = *reinterpret_cast<const float4*>(x + ((((long long)n * H + hi) * W + wi) * C4 + c4) * 4);
                const unsigned char p = (unsigned char)(a * 3 + b);
                if (v.x > m.x || k.x == 255) { m.x = v.x; k.x = p; }        // strictly greater: the first maximum stays
                if (v.y > m.y || k.y == 255) { m.y = v.y; k.y = p; }
                if (v.z > m.z || k.z == 255) { m.z = v.z; k.z = p; }
                if (v.w > m.w || k.w == 255) { m.w = v.w; k.w = p; }
            }
        }
        *reinterpret_cast<float4*>(y + g * 4) = m;
        idx[g] = k;
        if (sh1 > 0.f) {
            uint2 hh_, ll_;
            split2_f16(m, sh1, hh_, ll_);
            y_h1[g] = hh_;
        }
    }
}

// Backward of that pool (+ the stem's ReLU gate): a pixel collects the gradient of every window (<= 4) whose recorded first maximum it
// is (ties: the first maximum in row-major window order, as TF's MaxPoolGrad), windows added in ascending (ho, wo) order: ~5 loads
// per pixel.
__global__ __launch_bounds__(256) void maxpool_bwd_idx_kernel(const float* __restrict__ c1, const float* __restrict__ dpool,
                                                              const uchar4* __restrict__ idx, int N, int H, int W, int C, int Ho, int Wo,
                                                              int pt, int pl, float* __restrict__ dc1) {
    const int C4 = C >> 2;
    const long long total = (long long)N * H * W * C4;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(g % C4);
        long long r = g / C4;
        const int wi = (int)(r % W);
        r /= W;
        const int hi = (int)(r % H);
        const int n = (int)(r / H);
        // c1 == nullptr (16-bit tier, fused root block): no conv1 map; dpool is already zero wherever the window's maximum is not positive
        const float4 v = c1 ? *reinterpret_cast<const float4*>(c1 + g * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v.x > 0.f || v.y > 0.f || v.z > 0.f || v.w > 0.f) {
            for (int ho = max(0, (hi + pt - 2 + 1) / 2); ho <= min(Ho - 1, (hi + pt) / 2); ++ho)
                for (int wo = max(0, (wi + pl - 2 + 1) / 2); wo <= min(Wo - 1, (wi + pl) / 2); ++wo) {
                    const long long o = (((long long)n * Ho + ho) * Wo + wo) * C4 + c4;
                    const uchar4 k = idx[o];
                    const unsigned char me = (unsigned char)((hi - (ho * 2 - pt)) * 3 + (wi - (wo * 2 - pl)));
                    if (k.x != me && k.y != me && k.z != me && k.w != me) continue;
                    const float4 d = *reinterpret_cast<const float4*>(dpool + o * 4);
                    if (k.x == me) acc.x += d.x;
                    if (k.y == me) acc.y += d.y;
                    if (k.z == me) acc.z += d.z;
                    if (k.w == me) acc.w += d.w;
                }
            if (!(v.x > 0.f)) acc.x = 0.f;        // ReLU gate of the stem
            if (!(v.y > 0.f)) acc.y = 0.f;
            if (!(v.z > 0.f)) acc.z = 0.f;
            if (!(v.w > 0.f)) acc.w = 0.f;
        }
        *reinterpret_cast<float4*>(dc1 + g * 4) = acc;
    }
}

struct TPlan {
    // retained activations
    size_t p0, c1, pool, pidx;
    std::vector<size_t> sc, r1, r2, xo;         // per unit
    size_t scmap, locref;
    // gradients
    size_t g0, g1, dxa, dr1, dr2, dxa_b, dr1_b, dr2_b, dc1, dph0, dph1, dwraw, colsum, tail;      // (_b: second copies, units alternate)
    // per-layer weight-gradient scratch (non-head layers): [colsum | dot][dWraw], one contiguous region zeroed once per backward pass
    std::vector<size_t> cs_l, dw_l;
    size_t dwall = 0, dwall_bytes = 0;
    // fp16 high / low copies (ConvArgs::shadow) of the tensors the 128 x 128 weight-gradient tiles read; 0: none
    std::vector<size_t> sh_r1, sh_r2, sh_xo;
    size_t sh_g0 = 0, sh_g1 = 0, sh_dr1 = 0, sh_dr2 = 0, sh_dr1_b = 0, sh_dr2_b = 0;
    size_t feat32 = 0;           // fast pass: fp32 copy of the block4 features for the heads' backward
    size_t dphh = 0;             // 16-bit tier: both heads' gathered loss gradients as one H1 tensor [B*h*w, heads_ct(nj)]
    size_t sh_pool = 0;          // 16-bit tier: H1 copy of the pool output (input of the first unit)
    size_t total;
};

size_t al(size_t x) { return (x + 255) / 256 * 256; }

TPlan make_tplan(const dgp_trainer* tr, int B) {
    const dgp_net* net = tr->net; const dgp_net_desc& d = net->desc;
    TPlan p;
    size_t o = 0;
    auto take = [&](size_t nfl) { size_t r = o; o += al(nfl * sizeof(float)); return r; };
    p.p0 = take((size_t)B * d.in_h * d.in_w * 4);
    p.c1 = take((size_t)B * net->h1 * net->w1 * 64);
    p.pool = take((size_t)B * net->hp * net->wp * 64);
    p.pidx = take((size_t)B * net->hp * net->wp * 64 / 4);      // uchar4 per window and 4 channels: first-maximum positions of the pool
    int h = net->hp, w = net->wp;
    size_t xmax = (size_t)B * h * w * 64, r1max = 0, r2max = 0;
    for (const Unit& u : net->units) {
        const int ho = u.ho, wo = u.wo;
        p.sc.push_back(u.sc >= 0 ? take((size_t)B * ho * wo * u.depth) : 0);
        p.r1.push_back(take((size_t)B * h * w * u.depth_bn));
        p.r2.push_back(take((size_t)B * ho * wo * u.depth_bn));
        p.xo.push_back(take((size_t)B * ho * wo * u.depth));
        xmax = std::max(xmax, (size_t)B * h * w * u.depth_in);
        xmax = std::max(xmax, (size_t)B * ho * wo * u.depth);
        r1max = std::max(r1max, (size_t)B * h * w * u.depth_bn);
        r2max = std::max(r2max, (size_t)B * ho * wo * u.depth_bn);
        h = ho; w = wo;
    }
    const int nj = d.num_joints;
    p.scmap = take((size_t)B * 4 * h * w * nj);
    p.locref = take((size_t)B * 4 * h * w * 2 * nj);
    p.g0 = take(xmax); p.g1 = take(xmax); p.dxa = take(xmax);
    p.dr1 = take(r1max); p.dr2 = take(r2max);
    p.dxa_b = take(xmax); p.dr1_b = take(r1max); p.dr2_b = take(r2max);
    p.dc1 = take((size_t)B * net->h1 * net->w1 * 64);
    p.dph0 = take((size_t)B * h * w * next_pow2(4 * nj));
    p.dph1 = take((size_t)B * h * w * next_pow2(8 * nj));
    p.dphh = take((size_t)B * h * w * heads_ct(nj) / 2);
    size_t wmax = 0;
    for (size_t li = 0; li < net->layers.size(); ++li) {
        const ConvLayer& l = net->layers[li];
        const int cdy = tr->tl[li].cpad ? tr->tl[li].cpad : l.Cout;
        wmax = std::max(wmax, (size_t)l.KH * l.KW * l.Cin * cdy);
    }
    p.colsum = take(2 * 4096);      // directly in front of dwraw: wgrad_launch zeroes both with one memset
    p.dwraw = take(wmax);
    p.tail = take(TAIL_SLAB_FLOATS);
    p.dwall = o;
    p.cs_l.assign(net->layers.size(), 0); p.dw_l.assign(net->layers.size(), 0);
    for (size_t li = 0; li < net->layers.size(); ++li) {
        if ((int)li == net->head_part || (int)li == net->head_locref) continue;
        const ConvLayer& l = net->layers[li];
        p.cs_l[li] = take((size_t)2 * l.Cout);
        p.dw_l[li] = take((size_t)l.KH * l.KW * l.Cin * l.Cout);
    }
    p.dwall_bytes = o - p.dwall;
    p.sh_r1.assign(net->units.size(), 0); p.sh_r2.assign(net->units.size(), 0); p.sh_xo.assign(net->units.size(), 0);
    if (g_wgrad_dma) {
        int hh = net->hp, ww = net->wp;
        for (size_t ui = 0; ui < net->units.size(); ++ui) {
            const Unit& u = net->units[ui];
            const int ho = u.ho, wo = u.wo;
            // a copy pays where a 128 x 128 tile reads it: r1 feeds conv2 (K = 9 C1, Cdy = C1), r2 feeds conv3, xo the next unit's conv1 / shortcut
            if (u.depth_bn >= 128) p.sh_r1[ui] = take((size_t)B * hh * ww * u.depth_bn);
            if (u.depth_bn >= 128) p.sh_r2[ui] = take((size_t)B * ho * wo * u.depth_bn);
            if (ui + 1 < net->units.size() && net->units[ui + 1].depth_bn >= 128) p.sh_xo[ui] = take((size_t)B * ho * wo * u.depth);
            hh = ho; ww = wo;
        }
        p.sh_g0 = take(xmax); p.sh_g1 = take(xmax);
        p.sh_dr1 = take(r1max); p.sh_dr2 = take(r2max); p.sh_dr1_b = take(r1max); p.sh_dr2_b = take(r2max);
        p.feat32 = take((size_t)B * h * w * net->units.back().depth);
        p.sh_pool = take((size_t)B * net->hp * net->wp * 64 / 2);
    }
    p.total = o;
    return p;
}

__global__ __launch_bounds__(256) void range_merge_kernel(float* __restrict__ a, const float* __restrict__ b, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const float x = a[i], y = b[i]; a[i] = (y > x || y != y) ? y : x; }      // non-negative maxima; a NaN stays
}

// start of a pass: prev <- pool over [n_copy) floats (what the same kind of pass measured one step ago), pool <- 0 over [n_zero) floats,
// optionally *flag <- 0 -- one launch instead of a copy and two fills (blit launches cost ~15 us of queue gaps each at the step's boundary)
__global__ __launch_bounds__(256) void range_roll_kernel(float* __restrict__ pool, float* __restrict__ prev, int n_copy, int n_zero, int* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_copy) prev[i] = pool[i];
    if (i < n_zero) pool[i] = 0.f;
    if (i == 0 && flag) *flag = 0;
}

// Start of a forward or a backward pass.  Forward: everything fresh (first half of the pool).  Backward: the forward tensors'
// ranges stay (weight gradients read the retained activations), gradient tensors take slots from the second half.
static void range_pass_begin(dgp_trainer* tr, hipStream_t s, bool backward, int* flag_to_clear = nullptr) {
    static const bool enabled = (dgp_tune("DGP_TRAIN_F16", 1) != 0) && conv_mode() == ConvMode::F16x3;
    RangeCtx& rng = tr->ctx.rng;
    rng.on = enabled && tr->d_rng_pool && tr->d_wrng;
    rng.pool = tr->d_rng_pool;
    const size_t fwd_bytes = (size_t)(2 * RANGE_FWD) * ABSMAX_SLOTS * sizeof(float);
    const size_t bwd_bytes = (size_t)(RANGE_POOL - 2 * RANGE_FWD) * ABSMAX_SLOTS * sizeof(float);
    rng.chain2 = false;
    if (!backward) { rng.slots.clear(); rng.slots2.clear(); rng.next = 0; rng.next2 = 0; rng.limit = RANGE_FWD; }
    else { rng.next = 2 * RANGE_FWD; rng.limit = RANGE_POOL; }
    rng.prev = tr->d_rng_prev;
    if (!backward) tr->ctx.shadow_prev.clear();
    if (!rng.on) return;
    // what this kind of pass measured one step ago predicts the scales of this pass's fp16 copies (chain 2's own slots are not needed:
    // after the merge chain 1's hold the maxima of the whole tensors)
    {
        const size_t off = (backward ? fwd_bytes : 0) / sizeof(float);
        const int n_copy = (g_wgrad_dma && tr->d_rng_prev) ? (int)((backward ? bwd_bytes : fwd_bytes / 2) / sizeof(float)) : 0;
        const int n_zero = (int)((backward ? bwd_bytes : fwd_bytes) / sizeof(float));
        hipLaunchKernelGGL(range_roll_kernel, dim3((n_zero + 255) / 256), dim3(256), 0, s, tr->d_rng_pool + off,
                           tr->d_rng_prev ? tr->d_rng_prev + off : nullptr, n_copy, n_zero, flag_to_clear);
    }
    if (backward) return;
    const size_t nl = tr->net->layers.size();
    for (size_t li = 0; li < nl; ++li) {
        if (tr->net->layers[li].d_w) rng.slots[tr->net->layers[li].d_w] = tr->d_wrng + li * ABSMAX_SLOTS;
        if (tr->tl[li].d_wT) rng.slots[tr->tl[li].d_wT] = tr->d_wrng + (nl + li) * ABSMAX_SLOTS;
    }
    if (tr->d_hmT && tr->d_hm_rng) rng.slots[tr->d_hmT] = tr->d_hm_rng;
}

// first unit whose tensors a fast pass keeps as cells: the first one with a 128-channel bottleneck (block2; its input is the fp16 copy --
// ConvArgs::shadow -- of block1's output), or EVERY unit for an H1 pass (16-bit tier: the first one reads the H1 copy of the pool output)
size_t first_cell_unit(const dgp_net* net, const TPlan& pl, bool h1) {
    if (h1 && pl.sh_pool) return 0;
    for (size_t ui = 1; ui < net->units.size(); ++ui)
        if (net->units[ui].depth_bn >= 128 && pl.sh_xo[ui - 1]) return ui;
    return net->units.size();
}

// Weight gradients beside the data-gradient chain of a backward pass (TrainCtx::s2).  readers: events recorded on s2 behind the launches
// that READ a gradient buffer -- the chain waits for them before it overwrites that buffer.
struct WgradSide {
    TrainCtx* c = nullptr;
    hipStream_t s = nullptr;                     // the chain's stream
    bool on = false;
    std::multimap<const void*, hipEvent_t> readers;
    void begin(TrainCtx* ctx, hipStream_t chain) { c = ctx; s = chain; on = true; c->ev_next = 0; }
    // st <- the stream for a launch that may run beside the chain: s2 behind everything enqueued on the chain's stream so far, or the chain's
    int fork(hipStream_t& st) {
        st = s;
        if (!on) return DGP_OK;
        hipEvent_t ready = c->take_event();
        if (!ready) return fail(DGP_ERR_HIP, "weight-gradient stream: hipEventCreate failed");
        HIP_TRY(hipEventRecord(ready, s));
        HIP_TRY(hipStreamWaitEvent(c->s2, ready, 0));
        st = c->s2;
        return DGP_OK;
    }
    // everything enqueued on s2 so far reads `buf`
    int reads(const void* buf) {
        hipEvent_t done = c->take_event();
        if (!done) return fail(DGP_ERR_HIP, "weight-gradient stream: hipEventCreate failed");
        HIP_TRY(hipEventRecord(done, c->s2));
        readers.emplace(buf, done);
        return DGP_OK;
    }
    // the chain is about to overwrite `buf`: wait for the weight-gradient launches that still read it
    hipError_t before_write(const void* buf) {
        if (!on) return hipSuccess;
        auto range = readers.equal_range(buf);
        for (auto it = range.first; it != range.second; ++it) {
            hipError_t e2 = hipStreamWaitEvent(s, it->second, 0);
            if (e2 != hipSuccess) return e2;
        }
        readers.erase(range.first, range.second);
        return hipSuccess;
    }
    // the chain's stream waits for every weight gradient (before the finalisation launches, and on every exit path)
    void join() {
        if (!on) return;
        on = false;
        readers.clear();
        hipEvent_t e = c->take_event();
        if (e && hipEventRecord(e, c->s2) == hipSuccess) (void)hipStreamWaitEvent(s, e, 0);
        else (void)hipStreamSynchronize(c->s2);
    }
    ~WgradSide() { join(); }
};

// One pass of the training step: a stack object of dgp_train_forward / dgp_train_backward, handed to everything that launches.
struct TrainPass {
    dgp_trainer* tr; TrainCtx& ctx; const dgp_net* net; const TPlan& pl;
    hipStream_t s;                  // the caller's stream
    char* ws;                       // workspace base
    int B;
    bool fast = false;              // units >= ub keep their tensors as cells with predicted scales (dgp_trainer_fast_mode)
    int fmt = 1;                    // cell format of the pass: 1 H2 (high / low), 2 H1 (tier 1: high only)
    size_t ub = 0;
    float* slab = nullptr;          // K-split slab for the launches of the running chain (null: forward chain 2)
    bool stem_fused = false;        // forward: the root block as the inference engine's one kernel
    // backward
    WgradSide side;
    struct { const FinDesc* tab = nullptr; int max_cout = 0, max_krows = 0; } fin;      // grids of the deferred finalisation's table launches
    float *G[2] = {nullptr, nullptr}, *GH[2] = {nullptr, nullptr};      // d loss / d (unit output), ping-pong: fp32 | as H1 tensors (tier 1)
    int cur = 0;
    bool heads_h1 = false, stem_wgrad_h1 = false;
    const float *stem_g = nullptr, *stem_g_prev = nullptr;              // unit 0's data gradient left as an H1 tensor for stem_wgrad_h1_kernel
    size_t grp_next = 0;            // next gradient group to complete
    TrainPass(dgp_trainer* t, hipStream_t st, void* workspace, const TPlan& p, int nt)
        : tr(t), ctx(t->ctx), net(t->net), pl(p), s(st), ws((char*)workspace), B(nt) { slab = F(p.tail); }
    float* F(size_t off) const { return (float*)(ws + off); }
    bool h1p() const { return fast && fmt == 2; }              // every tensor of units >= ub is H1-only
    int copy_fmt() const { return h1p() ? 2 : 1; }             // format of the fp16 copies (ConvArgs::shadow) written in this pass
    int nu() const { return (int)net->units.size(); }
};

}  // namespace

// layer l as a forward conv x [N, H, W, l.Cin] -> y [N, Ho, Wo, l.Cout]
static dgp_conv_desc layer_desc(const ConvLayer& l, int N, int H, int W, int Ho, int Wo, int stride = 1, int pad_t = 0, int pad_l = 0) {
    dgp_conv_desc d{};
    d.N = N; d.H = H; d.W = W; d.Cin = l.Cin; d.Ho = Ho; d.Wo = Wo; d.Cout = l.Cout;
    d.KH = l.KH; d.KW = l.KW; d.stride = stride; d.rate = l.rate; d.pad_t = pad_t; d.pad_l = pad_l;
    return d;
}
// forward conv of layer l on the input's own grid: its panel, BN affine, ReLU
static ConvCall conv_call(const ConvLayer& l, const float* in, int N, int H, int W, float* out) {
    ConvCall c;
    c.d = layer_desc(l, N, H, W, H, W);
    c.d.relu = 1;
    c.wpk = l.d_w; c.nk = l.nk; c.coutP = l.CoutP; c.scale = l.has_bn ? l.d_scale : nullptr; c.bias = l.d_bias;
    c.in = in; c.out = out;
    return c;
}

ConvCall dgrad_call(const dgp_conv_desc& f, const float* wT, int nkT, int cinP, const float* dy, float* dx, bool stuffed) {
    ConvCall c;
    const int keff_h = (f.KH - 1) * f.rate + 1, keff_w = (f.KW - 1) * f.rate + 1;
    const int z = stuffed ? f.stride : 1;
    c.d.N = f.N; c.d.H = z * f.Ho; c.d.W = z * f.Wo; c.d.Cin = f.Cout; c.d.Ho = f.H; c.d.Wo = f.W; c.d.Cout = f.Cin;
    c.d.KH = f.KH; c.d.KW = f.KW; c.d.stride = 1; c.d.rate = f.rate;
    c.d.pad_t = keff_h - 1 - f.pad_t; c.d.pad_l = keff_w - 1 - f.pad_l;
    c.up = (!stuffed && f.stride > 1) ? f.stride : 0;
    c.wpk = wT; c.nk = nkT; c.coutP = cinP;
    c.in = dy; c.out = dx;
    return c;
}
// ... of a layer of the net, through the panel the weight sync packed
static ConvCall dgrad_call(const dgp_conv_desc& fwd, const TLayer& t, const float* dy, float* dx, bool stuffed = false) {
    return dgrad_call(fwd, t.d_wT, t.nkT, t.cinP, dy, dx, stuffed);
}

int conv_args(ConvArgs& a, const ConvCall& c, const char* too_big) {
    a.in = c.in; a.wpk = c.wpk; a.scale = c.scale; a.bias = c.bias; a.res = c.res; a.mask = c.mask; a.out = c.out;
    if (int rc = fill_conv_geometry(a, c.d, too_big)) return rc;       // 32-bit buffer descriptors: every tensor stays below 4 GiB
    a.CoutP = c.coutP; a.nk = c.nk; a.w_bytes = (unsigned)((size_t)c.nk * 8 * c.coutP * 16);      // (the panel as the trainer packed it)
    a.up = c.up; a.out_mode = c.out_mode; a.dc_nj = c.dc_nj;
    a.mask_fmt = c.mask_fmt; a.in_fmt = c.in_fmt; a.out_fmt = c.out_fmt; a.res_fmt = c.res_fmt;
    return DGP_OK;
}

// the launch inside a pass: range slots by tensor name, the panel's cells, predicted scales, the fp16 copy of the output
static hipError_t conv_launch(TrainPass& p, const ConvCall& c, hipStream_t s) {
    TrainCtx& ctx = p.ctx; RangeCtx& rng = ctx.rng;
    ConvArgs a{};
    if (conv_args(a, c, TOO_BIG)) return hipErrorInvalidValue;         // (lower the batch)
    a.slab = p.slab; a.slab_bytes = p.slab ? (unsigned)(TAIL_SLAB_FLOATS * sizeof(float)) : 0u;
    const int out_mode = c.out_mode;
    const float* rin = rng.of(c.in_key ? c.in_key : c.in);
    const float* rw = rng.of(c.wpk);
    if (c.in_fmt || c.out_fmt || c.res_fmt) {
        if (!(rin && rw && out_mode == 0 && c.in_fmt && c.out_fmt == c.in_fmt && (!c.res_fmt || c.res_fmt == c.in_fmt))) return hipErrorInvalidValue;
        a.in_scale_dev = rng.prev_of(rin);
        if (c.res_fmt) a.res_scale_dev = rng.prev_of(rng.of(c.res_key));
        if (!a.in_scale_dev || (c.res_fmt && !a.res_scale_dev)) return hipErrorInvalidValue;
    }
    if (rin && rw && out_mode == 0) {
        a.in_absmax = rin; a.w_absmax = rw;
        const auto cl = ctx.cells.find(c.wpk);
        if (g_train_cells && cl != ctx.cells.end()) { a.wh3 = cl->second; a.wh3_bytes = a.w_bytes; }
        if (a.in_fmt == 2) {                       // H1 operands: the panel's high-only cells (none: launch_conv refuses)
            const auto c1 = ctx.cells1.find(c.wpk);
            a.wh3 = c1 != ctx.cells1.end() ? c1->second : nullptr;
            a.wh3_bytes = a.w_bytes;               // (fp32-panel bytes: launch_conv halves both for H1 cells)
        }
    }
    const void* key = c.out_key ? c.out_key : (const void*)c.out;
    if (out_mode == 0) {
        a.out_absmax = rng.take();
        rng.set(key, a.out_absmax);
    }
    const int tile = pick_tile(a.M, a.CoutP, a.nk * BK, a.in_absmax && a.w_absmax);
    if (a.out_fmt) {
        // the output IS the fp16 high / low tensor: later weight-gradient launches read it in place
        a.out_scale_dev = rng.prev_of(a.out_absmax);
        if (!a.out_scale_dev || !a.wh3) return hipErrorInvalidValue;
        ctx.note_cells(key, a.out_scale_dev);
    } else if (out_mode == 0) {
        // fp16 copy of the output for wgrad_dma: kernels that end in ls_epilogue / tail_fixup_kernel write it
        const auto sb = ctx.shadow_base.find(key);
        const float* prev = rng.prev_of(a.out_absmax);
        if (sb != ctx.shadow_base.end() && c.copy && prev && (tile == TILE_128x128_H3K32 || tile == TILE_128x64_H3) &&
            a.in_absmax && a.w_absmax && a.Cin >= 32 && a.Cout % 8 == 0) {
            const ptrdiff_t off = c.out - static_cast<const float*>(key);
            a.shadow_fmt = p.copy_fmt();
            a.shadow = a.shadow_fmt == 2 ? reinterpret_cast<float*>(reinterpret_cast<char*>(sb->second) + off * 2) : sb->second + off;
            a.shadow_prev = prev;
            ctx.shadow_prev[key] = prev;
        } else {
            ctx.shadow_prev.erase(key);
        }
    }
    return launch_conv(a, tile, s);
}

extern "C" {

int dgp_trainer_create(dgp_net* net, dgp_trainer** out) {
    if (!net || !out) return fail(DGP_ERR_INVALID, "dgp_trainer_create: null argument");
    if (net->head_locref < 0) return fail(DGP_ERR_INVALID, "dgp_trainer_create: the net must be built with_locref (dgp_loss trains both heads)");
    dgp_trainer* tr = new dgp_trainer();
    tr->net = net;
    net->owner = tr; net->owner_sync = trainer_owner_sync;
    tr->tl.resize(net->layers.size());
    auto add = [&](const std::string& name, long long size, bool stat) {
        long long& ctr = stat ? tr->n_stat : tr->n_train;
        const long long off = ctr;
        ctr += (size + 3) / 4 * 4;                 // keep every tensor 16-byte aligned
        tr->names.push_back(name); tr->offs.push_back(off); tr->sizes.push_back(size); tr->is_stat.push_back(stat ? 1 : 0);
        return off;
    };
    for (size_t li = 0; li < net->layers.size(); ++li) {
        const ConvLayer& l = net->layers[li];
        TLayer& t = tr->tl[li];
        const bool head = ((int)li == net->head_part || (int)li == net->head_locref);
        if (head) {
            const int njt = l.Cout / 4;
            t.cin_real = l.Cin;
            t.w_off = add(l.scope + "/weights", 9ll * njt * l.Cin, false);
            t.b_off = add(l.scope + "/biases", njt, false);
            t.cpad = next_pow2(l.Cout);
            t.cinP = coutp_for(l.Cin);
            t.nkT = nk_for(2, 2, t.cpad);
        } else {
            t.cin_real = ((int)li == net->conv1) ? 3 : l.Cin;
            t.w_off = add(l.scope + "/weights", (long long)l.KH * l.KW * t.cin_real * l.Cout, false);
            t.g_off = add(l.scope + "/BatchNorm/gamma", l.Cout, false);
            t.b_off = add(l.scope + "/BatchNorm/beta", l.Cout, false);
            t.mean_off = add(l.scope + "/BatchNorm/moving_mean", l.Cout, true);
            t.var_off = add(l.scope + "/BatchNorm/moving_variance", l.Cout, true);
            if ((int)li != net->conv1) {
                t.cinP = coutp_for(l.Cin);
                t.nkT = nk_for(l.KH, l.KW, l.Cout);
            }
        }
        if (t.nkT > 0) {
            if (hipMalloc(&t.d_wT, (size_t)t.nkT * 8 * t.cinP * 16) != hipSuccess) {
                delete tr;
                return fail(DGP_ERR_HIP, "dgp_trainer_create: hipMalloc (dgrad panels) failed");
            }
        }
    }
    const size_t nb = (size_t)tr->n_train * sizeof(float);
    if (hipMalloc(&tr->params, nb) != hipSuccess || hipMalloc(&tr->grads, nb) != hipSuccess ||
        hipMalloc(&tr->mom, nb) != hipSuccess || hipMalloc(&tr->stats, (size_t)tr->n_stat * sizeof(float)) != hipSuccess ||
        hipMalloc(&tr->d_sumsq, 2 * sizeof(double)) != hipSuccess || hipMalloc(&tr->d_gnorm, sizeof(float)) != hipSuccess ||
        hipMemset(tr->d_sumsq, 0, 2 * sizeof(double)) != hipSuccess || hipMemset(tr->d_gnorm, 0, sizeof(float)) != hipSuccess ||
        hipHostMalloc(&tr->h_status, 16 * sizeof(float), hipHostMallocDefault) != hipSuccess) {
        delete tr;
        return fail(DGP_ERR_HIP, "dgp_trainer_create: hipMalloc failed");
    }
    (void)hipMemset(tr->params, 0, nb); (void)hipMemset(tr->grads, 0, nb); (void)hipMemset(tr->mom, 0, nb);
    if (hipMalloc(&tr->d_rng_pool, (size_t)RANGE_POOL * ABSMAX_SLOTS * sizeof(float)) != hipSuccess ||
        hipMalloc(&tr->d_rng_prev, (size_t)RANGE_POOL * ABSMAX_SLOTS * sizeof(float)) != hipSuccess ||
        hipMalloc(&tr->d_fast_flag, sizeof(int)) != hipSuccess || hipMemset(tr->d_fast_flag, 0, sizeof(int)) != hipSuccess ||
        hipMemset(tr->d_rng_pool, 0, (size_t)RANGE_POOL * ABSMAX_SLOTS * sizeof(float)) != hipSuccess ||
        hipMemset(tr->d_rng_prev, 0, (size_t)RANGE_POOL * ABSMAX_SLOTS * sizeof(float)) != hipSuccess ||
        hipMalloc(&tr->d_wrng, (size_t)2 * net->layers.size() * ABSMAX_SLOTS * sizeof(float)) != hipSuccess) {
        delete tr;
        return fail(DGP_ERR_HIP, "dgp_trainer_create: hipMalloc failed");
    }
    *out = tr;
    return DGP_OK;
}

void dgp_trainer_destroy(dgp_trainer* tr) {
    if (tr && tr->net && tr->net->owner == tr) { tr->net->owner = nullptr; tr->net->owner_sync = nullptr; }      // (the net outlives its trainer: train.py)
    delete tr;
}

int dgp_trainer_num_tensors(const dgp_trainer* tr, int32_t* n_tensors, int64_t* n_trainable_floats, int64_t* n_stat_floats) {
    if (!tr) return fail(DGP_ERR_INVALID, "dgp_trainer_num_tensors: null");
    if (n_tensors) *n_tensors = (int32_t)tr->names.size();
    if (n_trainable_floats) *n_trainable_floats = tr->n_train;
    if (n_stat_floats) *n_stat_floats = tr->n_stat;
    return DGP_OK;
}

int dgp_trainer_tensor_info(const dgp_trainer* tr, int32_t i, char* name, int32_t cap, int64_t* offset, int64_t* size,
                            int32_t* is_stat) {
    if (!tr || i < 0 || i >= (int)tr->names.size()) return fail(DGP_ERR_INVALID, "dgp_trainer_tensor_info: bad index");
    if (name && cap > 0) { strncpy(name, tr->names[i].c_str(), cap - 1); name[cap - 1] = 0; }
    if (offset) *offset = tr->offs[i];
    if (size) *size = tr->sizes[i];
    if (is_stat) *is_stat = tr->is_stat[i];
    return DGP_OK;
}

/* which: 0 params, 1 grads, 2 momentum, 3 frozen statistics; 5 / 6 / 7: Adam's m, v and {beta1_power, beta2_power} -- NULL until allocated */
float* dgp_trainer_buffer(dgp_trainer* tr, int32_t which) {
    if (!tr) return nullptr;
    switch (which) {
        case 5: return tr->adam_m; case 6: return tr->adam_v;
        case 7: return tr->d_adam_pow ? tr->d_adam_pow + 2 * tr->adam_pow_k : nullptr;
        case 0: return tr->params; case 1: return tr->grads; case 2: return tr->mom; case 3: return tr->stats;
        case 4: return reinterpret_cast<float*>(tr->d_fast_flag);      // ONE int32: != 0 when a 16-bit pass left its predicted ranges (data-parallel: all-reduce MAX)
    }
    return nullptr;
}

int dgp_trainer_workspace_bytes(const dgp_trainer* tr, int32_t nt, size_t* out_bytes) {
    if (!tr || !out_bytes || nt < 1) return fail(DGP_ERR_INVALID, "dgp_trainer_workspace_bytes: bad argument");
    *out_bytes = make_tplan(tr, nt).total;
    return DGP_OK;
}

}  // extern "C"

// The root block's unfused pool of the training step and its backward, as forward_root / backward_root launch them (and the layer-level
// entry points dgp_maxpool_fwd_idx / dgp_maxpool_bwd_idx).  c1 [nB, h1, w1, 64] -> pool [nB, hp, wp, 64] + the first-maximum record;
// y_h1 / y_prev: the optional H1 copy and the range slots that predict its scale.
void launch_maxpool_fwd_idx(const float* c1, int nB, int h1, int w1, int hp, int wp, float* pool, uchar4* idx, uint2* y_h1, const float* y_prev,
                            hipStream_t s) {
    const long long totp = (long long)nB * hp * wp * 16;
    hipLaunchKernelGGL(maxpool_fwd_idx_kernel, dim3(grid_for(totp)), dim3(256), 0, s, c1, nB, h1, w1, 16, hp, wp, pool_pad_before(h1, hp),
                       pool_pad_before(w1, wp), pool, idx, y_h1, y_prev);
}
// c1 == nullptr: no ReLU gate (the 16-bit tier's fused root block keeps no conv1 map)
void launch_maxpool_bwd_idx(const float* c1, const float* dpool, const uchar4* idx, int B, int h1, int w1, int hp, int wp, float* dc1, hipStream_t s) {
    const long long tot = (long long)B * h1 * w1 * 16;
    hipLaunchKernelGGL(maxpool_bwd_idx_kernel, dim3(grid_for(tot)), dim3(256), 0, s, c1, dpool, idx, B, h1, w1, 64, hp, wp,
                       pool_pad_before(h1, hp), pool_pad_before(w1, wp), dc1);
}

// ---- the other element-wise kernels that the layer-level entry points launch as well (dgp_train.h) ----
void launch_f32_to_h1_pred(const float* x, long long n, const float* prev, void* out_h1, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_h1_pred_kernel, dim3(grid_for(n / 8)), dim3(256), 0, s, reinterpret_cast<const float4*>(x), n / 8, prev,
                       reinterpret_cast<uint4*>(out_h1));
}
void launch_h1_to_f32_pred(const void* x_h1, long long n8, const float* prev, float* out, const void* gate_h1, hipStream_t s) {
    hipLaunchKernelGGL(h1_to_f32_pred_kernel, dim3(grid_for(n8)), dim3(256), 0, s, reinterpret_cast<const uint4*>(x_h1), n8, prev,
                       reinterpret_cast<float4*>(out), reinterpret_cast<const uint4*>(gate_h1));
}
void launch_f32_to_shadow(const float* x, long long n8, const float* prev, void* out_h2, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_shadow_kernel, dim3(grid_for(n8)), dim3(256), 0, s, reinterpret_cast<const float4*>(x), n8, prev,
                       reinterpret_cast<uint4*>(out_h2));
}
// (materialised, a few MB, so that the data gradient of a stride-2 conv is a plain stride-1 launch of the cell kernels)
hipError_t h1_zero_stuff(hipStream_t s, const void* dy_h1, int N, int Ho, int Wo, int C, void* out) {
    hipError_t e = hipMemsetAsync(out, 0, (size_t)N * 2 * Ho * 2 * Wo * C * 2, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(h1_zero_stuff_kernel, dim3(grid_for((long long)N * Ho * Wo * (C / 8))), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(dy_h1), N, Ho, Wo, C / 8, reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}
int launch_h2_pred_check(const int* slots, int n, const float* pool, const float* prev, int* flag, const char* too_many, hipStream_t s) {
    H2CheckList cl{};
    if ((size_t)n > sizeof(cl.idx) / sizeof(cl.idx[0])) return fail(DGP_ERR_STATE, too_many);
    cl.n = n;
    for (int k = 0; k < n; ++k) cl.idx[k] = (short)slots[k];
    if (n) hipLaunchKernelGGL(h2_pred_check_kernel, dim3(n), dim3(64), 0, s, cl, pool, prev, flag);
    return DGP_OK;
}
void launch_head_gather_h1(const float* dsc0, const float* dsc1, int N, int h, int w, int njt0, int cpad0, int njt1, int cpad1, int CT,
                           const float* prev, void* out_h1, float* slot, hipStream_t s) {
    hipLaunchKernelGGL(head_gather_h1_kernel, dim3(grid_for((long long)N * h * w * (CT / 8))), dim3(256), 0, s, dsc0, dsc1, N, h, w, njt0, cpad0,
                       njt1, cpad1, CT, prev, reinterpret_cast<uint4*>(out_h1), slot);
}

// the trainer's second stream (least urgent priority), created on first use
static int ensure_side_stream(TrainCtx& ctx) {
    if (ctx.s2) return DGP_OK;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);         // lo: numerically greatest = least urgent
    HIP_TRY(hipStreamCreateWithPriority(&ctx.s2, hipStreamNonBlocking, lo));
    return DGP_OK;
}

// ---- the forward pass in stages: root block and bottleneck units per chain of frames, heads, the fast pass's check ----
// One chain of frames [n0, n0 + nB) on stream cs; (hh, ww, x_off, x_c): the grid, workspace offset and channels of the next unit's input
struct Chain { int n0, nB; hipStream_t cs; bool second; int hh, ww; size_t x_off; int x_c; };

// the launches that follow belong to chain c: its range slots, and the K-split slab for the first chain only
static void enter_chain(TrainPass& p, const Chain& c) {
    p.slab = c.second ? nullptr : p.F(p.pl.tail);
    p.ctx.rng.chain2 = c.second;
}

static int forward_root(TrainPass& p, const Chain& c, const uint8_t* frames) {
    enter_chain(p, c);
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; const TPlan& pl = p.pl; TrainCtx& ctx = p.ctx; RangeCtx& rng = ctx.rng;
    const dgp_net_desc& d = net->desc;
    const ConvLayer& c1 = net->layers[net->conv1];
    const int n0 = c.n0, nB = c.nB;
    hipStream_t cs = c.cs;
    auto at = [&](size_t off, size_t per_frame) { return p.F(off) + (size_t)n0 * per_frame; };
    const size_t px_in = (size_t)d.in_h * d.in_w, px1 = (size_t)net->h1 * net->w1, pxp = (size_t)net->hp * net->wp;
    HIP_TRY(launch_preprocess(frames + (size_t)n0 * px_in * 3, (long long)nB * d.in_h * d.in_w, d.mean_pixel[0], d.mean_pixel[1],
                              d.mean_pixel[2], at(pl.p0, px_in * 4), cs));
    if (p.stem_fused) {
        // 16-bit tier: the root block as the inference engine's ONE kernel (uint8 frame -> conv1 + BN + ReLU -> max-pool -> H1 cells of the
        // pool output, scale predicted from conv1's range one step ago) that also records each window's first maximum.  No conv1 map, no
        // fp32 pool output: the first unit reads the H1 tensor, the pool's backward needs only the record.  (The centred frame above
        // stays: the stem's weight gradient reads it.)  The launch takes conv1's range slot, in conv1's place in the order of slots.
        float* slot = rng.take();
        const float* yprev = rng.prev_of(slot);
        if (!slot || !yprev) return fail(DGP_ERR_STATE, "16-bit tier: the root block's output has no predicted range");
        rng.set(p.F(pl.c1), slot);
        rng.set(p.F(pl.pool), slot);
        ctx.shadow_base[p.F(pl.pool)] = p.F(pl.sh_pool);
        ctx.shadow_prev[p.F(pl.pool)] = yprev;
        HIP_TRY(launch_stem_pool_fused(frames + (size_t)n0 * px_in * 3, nB, d.in_h, d.in_w, tr->d_stem_cells,
                                       tr->d_wrng + (size_t)net->conv1 * ABSMAX_SLOTS, c1.d_scale, c1.d_bias, d.mean_pixel[0], d.mean_pixel[1],
                                       d.mean_pixel[2], 0.f, reinterpret_cast<float*>(reinterpret_cast<char*>(p.F(pl.sh_pool)) + (size_t)n0 * pxp * 64 * 2),
                                       slot, cs, 1, yprev, reinterpret_cast<unsigned char*>(p.ws + pl.pidx) + (size_t)n0 * pxp * 64));
        return DGP_OK;
    }
    HIP_TRY(conv_launch(p, conv_call(c1, at(pl.p0, px_in * 4), nB, d.in_h, d.in_w, at(pl.c1, px1 * 64)).grid(net->h1, net->w1, 3, 3).strided(2)
                               .keys(p.F(pl.p0), p.F(pl.c1)), cs));
    uint2* yh1 = nullptr;
    const float* yprev = nullptr;
    if (p.h1p() && p.ub == 0) {        // H1 copy of the pool output for the first unit (scale: conv1's range one step ago)
        yprev = rng.prev_of(rng.of(p.F(pl.c1)));
        if (!yprev) return fail(DGP_ERR_STATE, "16-bit tier: the root block's output has no predicted range");
        yh1 = reinterpret_cast<uint2*>(reinterpret_cast<char*>(p.F(pl.sh_pool)) + (size_t)n0 * pxp * 64 * 2);
        ctx.shadow_base[p.F(pl.pool)] = p.F(pl.sh_pool);
        ctx.shadow_prev[p.F(pl.pool)] = yprev;
    }
    launch_maxpool_fwd_idx(at(pl.c1, px1 * 64), nB, net->h1, net->w1, net->hp, net->wp, at(pl.pool, pxp * 64),
                           reinterpret_cast<uchar4*>(p.ws + pl.pidx) + (size_t)n0 * pxp * 16, yh1, yprev, cs);
    rng.set(p.F(pl.pool), rng.of(p.F(pl.c1)));      // max-pooling cannot raise the maximum
    return DGP_OK;
}

static int forward_unit(TrainPass& p, Chain& c, size_t ui) {
    enter_chain(p, c);
    const dgp_net* net = p.net; const TPlan& pl = p.pl;
    const int n0 = c.n0, nB = c.nB, hh = c.hh, ww = c.ww;
    hipStream_t cs = c.cs;
    const Unit& u = net->units[ui];
    const int ho = u.ho, wo = u.wo;
    const size_t pin = (size_t)hh * ww, pout = (size_t)ho * wo;
    const bool h2u = p.fast && ui >= p.ub;         // this unit's tensors are H2 / H1 cells
    const bool h1u = h2u && p.fmt == 2;
    // (the first H2 unit reads the fp16 copy of its fp32 input; ranges and scales go by the tensor's own name, F(c.x_off))
    // (frame offsets inside H1 tensors are half the fp32 ones: atf)
    auto atf = [&](size_t off, size_t per_frame, bool cells1) {
        return cells1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(p.F(off)) + (size_t)n0 * per_frame * 2) : p.F(off) + (size_t)n0 * per_frame;
    };
    // a launch of this unit: range keys, and on a fast pass the cell format of its tensors (rkey: the residual's tensor)
    auto launch = [&](ConvCall call, const void* in_key, const void* out_key, const void* rkey = nullptr) {
        call.keys(in_key, out_key);
        if (h2u) call.cells(p.fmt, rkey);
        return conv_launch(p, call, cs);
    };
    const float* x = (h2u && ui == p.ub) ? atf(ui == 0 ? pl.sh_pool : pl.sh_xo[ui - 1], pin * c.x_c, h1u) : atf(c.x_off, pin * c.x_c, h1u && ui > p.ub);
    float* const r1 = atf(pl.r1[ui], pin * u.depth_bn, h1u);
    float* const r2 = atf(pl.r2[ui], pout * u.depth_bn, h1u);
    const float* res = x;
    const void* res_key = p.F(c.x_off);
    int res_s = u.stride, res_H = hh, res_W = ww;
    if (u.sc >= 0) {
        float* const sc = atf(pl.sc[ui], pout * u.depth, h1u);
        HIP_TRY(launch(conv_call(net->layers[u.sc], x, nB, hh, ww, sc).grid(ho, wo).strided(u.stride).linear(), p.F(c.x_off), p.F(pl.sc[ui])));
        res = sc; res_s = 1; res_H = ho; res_W = wo;
        res_key = p.F(pl.sc[ui]);
    }
    HIP_TRY(launch(conv_call(net->layers[u.c1], x, nB, hh, ww, r1), p.F(c.x_off), p.F(pl.r1[ui])));
    HIP_TRY(launch(conv_call(net->layers[u.c2], r1, nB, hh, ww, r2).grid(ho, wo, u.pb_h, u.pb_w).strided(u.stride), p.F(pl.r1[ui]), p.F(pl.r2[ui])));
    HIP_TRY(launch(conv_call(net->layers[u.c3], r2, nB, ho, wo, atf(pl.xo[ui], pout * u.depth, h1u)).residual(res, res_s, res_H, res_W),
                   p.F(pl.r2[ui]), p.F(pl.xo[ui]), res_key));
    c.x_off = pl.xo[ui]; c.x_c = u.depth; c.hh = ho; c.ww = wo;
    return DGP_OK;
}

// one head on the features xin [B, h, w, Cin]: pointwise GEMM on the cell kernels + gather of the four taps (as the inference engine) when the
// feature map's range and the pointwise cells exist, else the 2x2-conv form on the fp32 kernel
static hipError_t forward_head(TrainPass& p, int li, int njt, const float* xin, int h, int w, float* out) {
    static const bool head_pw = (dgp_tune("DGP_HEAD_PW", 1) != 0);
    const dgp_trainer* tr = p.tr;
    const ConvLayer& hd = p.net->layers[li];
    const RangeCtx& rng = p.ctx.rng;
    const float* rin = rng.of(xin);
    const float* rw = tr->d_wrng ? tr->d_wrng + (size_t)li * ABSMAX_SLOTS : nullptr;
    if (p.fast && !(head_pw && rin && rw && hd.d_wh3_pw && tr->d_h3_table && (p.fmt == 1 || hd.d_wh1_pw))) return hipErrorInvalidValue;       // (H2 / H1 features: cell kernels only)
    if (!(head_pw && rng.on && rin && rw && hd.d_wh3_pw && tr->d_h3_table))
        return conv_launch(p, conv_call(hd, xin, p.B, h, w, out).grid(h, w, 1, 1).linear().head_scatter(njt), p.s);
    float* T = p.F(p.pl.g0);                       // gradient scratch: free during the forward pass
    ConvArgs a = head_pointwise_args(hd, xin, p.B, h, w, T, rin, rw);
    if (p.fast) {
        a.in_fmt = p.fmt; a.in_scale_dev = rng.prev_of(rin);
        if (!a.in_scale_dev) return hipErrorInvalidValue;
        if (p.fmt == 2) a.wh3 = hd.d_wh1_pw;
    }
    a.slab = p.slab; a.slab_bytes = p.slab ? (unsigned)(TAIL_SLAB_FLOATS * sizeof(float)) : 0u;
    hipError_t e = launch_conv(a, pick_tile(a.M, a.CoutP, a.nk * BK, true), p.s);
    if (e != hipSuccess) return e;
    return launch_head_gather(T, hd.d_bias, p.B, h, w, njt, hd.coutp_pw, out, p.s);
}

// every tensor of `ctx.h2_slots` against its predicted scale: raises the trainer's flag (the host repeats the step)
static int check_predictions(TrainPass& p, const char* too_many) {
    const std::vector<int>& slots = p.ctx.h2_slots;
    return launch_h2_pred_check(slots.data(), (int)slots.size(), p.ctx.rng.pool, p.ctx.rng.prev, p.tr->d_fast_flag, too_many, p.s);
}

// end of a fast forward pass: the check of its predicted scales, and the fp32 copy of the features for the heads' backward
static int forward_fast_tail(TrainPass& p, const float* xin, int h, int w) {
    dgp_trainer* tr = p.tr; TrainCtx& ctx = p.ctx; const TPlan& pl = p.pl;
    {   // every H2 tensor of this pass is checked against its predicted scale, and the fp16 copy of block1's output that the first H2 unit read
        const float* pv = ctx.rng.prev_of(ctx.rng.of(p.ub == 0 ? p.F(pl.pool) : p.F(pl.xo[p.ub - 1])));
        if (!pv) return fail(DGP_ERR_STATE, "fast pass: the first H2 unit's input has no range");
        ctx.h2_slots.push_back((int)((pv - ctx.rng.prev) / ABSMAX_SLOTS));
    }
    if (int rc = check_predictions(p, "fast pass: too many H2 tensors")) return rc;
    // fp32 copy of the features for the heads' backward (not when it reads the H1 features in place: merged heads of the 16-bit tier)
    const float* rfeat = ctx.rng.of(xin);
    const long long n8 = (long long)p.B * h * w * p.net->units.back().depth / 8;
    tr->fwd_feat32 = !(p.fmt == 2 && tr->d_hmT && tr->d_hmT_h1);
    if (!tr->fwd_feat32) {
    } else if (p.fmt == 2)
        launch_h1_to_f32_pred(xin, n8, ctx.rng.prev_of(rfeat), p.F(pl.feat32), nullptr, p.s);
    else
        hipLaunchKernelGGL(h2_to_f32_pred_kernel, dim3(grid_for(n8)), dim3(256), 0, p.s, reinterpret_cast<const uint4*>(xin), n8,
                           ctx.rng.prev_of(rfeat), reinterpret_cast<float4*>(p.F(pl.feat32)));
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

extern "C" int dgp_train_forward(dgp_trainer* tr, const uint8_t* frames, int32_t nt, void* workspace, size_t workspace_bytes,
                                 float** scmap, float** locref, void* stream) {
    if (!tr || !frames || !workspace) return fail(DGP_ERR_INVALID, "dgp_train_forward: null argument");
    dgp_net* net = tr->net;
    if (!net->loaded) return fail(DGP_ERR_STATE, "dgp_train_forward: call dgp_trainer_sync_weights first");
    const TPlan pl = make_tplan(tr, nt);
    if (workspace_bytes < pl.total) return fail(DGP_ERR_INVALID, "dgp_train_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    TrainPass p(tr, s, workspace, pl, nt);
    TrainCtx& ctx = p.ctx;
    range_pass_begin(tr, s, false, tr->d_fast_flag);      // (also clears the range flag of a fast pass: fast needs the ranges on)
    ctx.shadow_base.clear();
    ctx.h2_slots.clear();
    // Fast pass (dgp_trainer_fast_mode; the host asks for it once a pass of the same shapes has left its ranges behind): from unit ub on every
    // retained activation is an H2 tensor -- fp16 high / low cells with a scale predicted from the previous step's range, no fp32 twin -- so
    // these convs run the inference engine's cell kernels (no split in the K loop, no second copy) and the weight gradients read them in place
    const size_t nu = net->units.size();
    p.ub = first_cell_unit(net, pl, tr->tier == 1);
    p.fmt = tr->tier == 1 ? 2 : 1;
    p.fast = tr->fast_next && g_wgrad_dma && g_train_cells && ctx.rng.on && p.ub < nu && pl.feat32 && (tr->tier != 1 || tr->d_h1_table);
    tr->fwd_fast = p.fast;
    tr->fwd_fmt = p.fast ? p.fmt : 0;
    if (!p.fast && tr->parity_stale) {           // a plain pass after lazy syncs: its panels first
        const int rcp = refresh_parity_panels(tr, s);
        if (rcp) return rcp;
    }
    for (size_t ui = 0; ui < nu; ++ui) {
        if (p.fast && ui >= p.ub) continue;          // (H2 tensors register themselves as they are written)
        if (pl.sh_r1[ui]) ctx.shadow_base[p.F(pl.r1[ui])] = p.F(pl.sh_r1[ui]);
        if (pl.sh_r2[ui]) ctx.shadow_base[p.F(pl.r2[ui])] = p.F(pl.sh_r2[ui]);
        if (pl.sh_xo[ui]) ctx.shadow_base[p.F(pl.xo[ui])] = p.F(pl.sh_xo[ui]);
    }
    const dgp_net_desc& d = net->desc;
    const int B = nt;
    // The forward pass as TWO chains of frames (DGP_FWD_CHAINS=1: one): frames [0, n1) on the caller's stream, [n1, B) on the trainer's
    // second stream.  At 11 frames the grids of block3 / block4 cover half of the chip, and two independent chains drift apart so that
    // one chain's small or tail-heavy layers run under the other's.  Both chains write frame ranges of the SAME activation tensors
    // (the backward pass sees one batch) and max into the same range slots.
    static const bool side_env = (dgp_tune("DGP_WGRAD_OVERLAP", 1) != 0);
    static const int chains_env = dgp_tune("DGP_FWD_CHAINS", 2);
    if (side_env)
        if (int rc = ensure_side_stream(ctx)) return rc;
    ctx.ev_next = 0;                             // (the previous backward pass has joined: its events are free again)
    const bool two = side_env && ctx.s2 && chains_env >= 2 && B >= 4;
    const int n1 = two ? (B + 1) / 2 : B;
    const ConvLayer& c1 = net->layers[net->conv1];
    p.stem_fused = p.h1p() && p.ub == 0 && tr->d_stem_cells && tr->d_wrng && c1.d_scale && c1.d_bias;
    tr->fwd_stem_fused = p.stem_fused;
    if (two) {
        hipEvent_t ready = ctx.take_event();
        if (!ready) return fail(DGP_ERR_HIP, "forward chains: hipEventCreate failed");
        HIP_TRY(hipEventRecord(ready, s));       // frames, weights and the zeroed range slots are in place
        HIP_TRY(hipStreamWaitEvent(ctx.s2, ready, 0));
    }
    // host enqueue order: stage by stage, chain 0 then chain 1 (a chain enqueued whole before the other would start a millisecond late)
    Chain chains[2] = {{0, n1, s, false, net->hp, net->wp, pl.pool, 64}, {n1, B - n1, ctx.s2, true, net->hp, net->wp, pl.pool, 64}};
    const int nchains = two ? 2 : 1;
    int rc;
    for (int ci = 0; ci < nchains; ++ci) if ((rc = forward_root(p, chains[ci], frames))) return rc;
    for (size_t ui = 0; ui < nu; ++ui)
        for (int ci = 0; ci < nchains; ++ci) if ((rc = forward_unit(p, chains[ci], ui))) return rc;
    enter_chain(p, chains[0]);
    if (two) {
        hipEvent_t done = ctx.take_event();
        if (!done) return fail(DGP_ERR_HIP, "forward chains: hipEventCreate failed");
        HIP_TRY(hipEventRecord(done, ctx.s2));
        HIP_TRY(hipStreamWaitEvent(s, done, 0));
        if (ctx.rng.on && ctx.rng.next2 > 0) {      // ranges of the whole tensors = max of the chains' (same slot order)
            if (ctx.rng.next2 != ctx.rng.next) return fail(DGP_ERR_STATE, "forward chains took different numbers of range slots");
            const int nfl = ctx.rng.next2 * ABSMAX_SLOTS;
            hipLaunchKernelGGL(range_merge_kernel, dim3((nfl + 255) / 256), dim3(256), 0, s, ctx.rng.pool,
                               ctx.rng.pool + (size_t)RANGE_FWD * ABSMAX_SLOTS, nfl);
        }
    }
    const int h = net->fh, w = net->fw;
    const float* xin = p.F(pl.xo[nu - 1]);
    HIP_TRY(forward_head(p, net->head_part, d.num_joints, xin, h, w, p.F(pl.scmap)));
    HIP_TRY(forward_head(p, net->head_locref, 2 * d.num_joints, xin, h, w, p.F(pl.locref)));
    if (p.fast && (rc = forward_fast_tail(p, xin, h, w))) return rc;
    if (scmap) *scmap = p.F(pl.scmap);
    if (locref) *locref = p.F(pl.locref);
    return DGP_OK;
}

// ---- the backward pass in stages ----
struct MapRef { const float* p; int H, W; };        // an NHWC tensor of the batch on its grid

// One conv layer's parameter gradients: dWraw = A^T dY, d beta = colsum(dY), then the BN-affine algebra.
// Every non-head layer accumulates dWraw / colsum in its own region of the workspace (zeroed once per pass; TPlan::dw_l / cs_l) and two
// table launches at the end of the pass turn them into dW, d gamma, d beta for all layers -- ~150 dispatches fewer per step than
// fill + fill + wgrad + scale + bn per layer.  side: beside the chain (WgradSide) where the pass overlaps.
static int layer_param_grads(TrainPass& p, size_t li, MapRef x, MapRef dy, int stride = 1, int pad_t = 0, int pad_l = 0, bool side = true) {
    dgp_trainer* tr = p.tr; TrainCtx& ctx = p.ctx;
    const ConvLayer& l = p.net->layers[li];
    hipStream_t st = p.s;
    const bool beside = side && p.side.on;
    if (beside)
        if (int rc = p.side.fork(st)) return rc;
    WgradCall c;
    c.d.N = p.B; c.d.H = x.H; c.d.W = x.W; c.d.Cin = l.Cin; c.d.Ho = dy.H; c.d.Wo = dy.W; c.d.Cout = l.Cout;
    c.d.KH = l.KH; c.d.KW = l.KW; c.d.stride = stride; c.d.rate = l.rate; c.d.pad_t = pad_t; c.d.pad_l = pad_l;
    c.x = {x.p, ctx.rng.of(x.p)};
    c.dy = {dy.p, ctx.rng.of(dy.p)};
    c.dwraw = reinterpret_cast<float*>(p.ws + p.pl.dw_l[li]);
    c.colsum = reinterpret_cast<float*>(p.ws + p.pl.cs_l[li]);
    c.zeroed = true;
    {
        const auto px = ctx.shadow_prev.find(x.p), py = ctx.shadow_prev.find(dy.p);
        const auto bx = ctx.shadow_base.find(x.p), by = ctx.shadow_base.find(dy.p);
        if (px != ctx.shadow_prev.end() && py != ctx.shadow_prev.end() && bx != ctx.shadow_base.end() && by != ctx.shadow_base.end()) {
            c.x.cells = bx->second; c.x.prev = px->second;
            c.dy.cells = by->second; c.dy.prev = py->second;
        }
    }
    if (c.x.cells && c.x.cells == (const void*)x.p) c.fail_flag = tr->d_fast_flag;      // fast pass: the activation has no fp32 twin
    c.h1 = p.h1p() && c.x.cells && c.dy.cells;                                          // 16-bit tier: both operands are H1 tensors
    if (c.h1) c.fail_flag = tr->d_fast_flag;
    if (!c.fail_flag && p.fast && ctx.shadow_base.count(x.p) && ctx.shadow_base[x.p] == x.p)
        return fail(DGP_ERR_STATE, "weight gradient of an H2-only activation without a usable gradient copy");
    HIP_TRY(wgrad_launch(c, st));
    if (beside) return p.side.reads(dy.p);
    return DGP_OK;
}

// (the pass: through the shared dwraw / colsum scratch of the plan; c.d is also the forward desc of the head's data gradient)
WgradCall head_wgrad_call(int N, int h, int w, int cin, int cdy, float* dwraw, float* colsum) {
    WgradCall c;
    c.d.N = N; c.d.H = c.d.Ho = h; c.d.W = c.d.Wo = w; c.d.Cin = cin; c.d.Cout = cdy;
    c.d.KH = c.d.KW = 2; c.d.stride = c.d.rate = 1; c.d.pad_t = c.d.pad_l = 1;
    c.dwraw = dwraw; c.colsum = colsum;
    return c;
}

// the deferred finalisation of `count` rows of the table from `first` on stream st: dW from dWraw, then d gamma / d beta
static void finalise(TrainPass& p, int first, int count, hipStream_t st) {
    if (count <= 0) return;
    const int rpb = 128;
    hipLaunchKernelGGL(scale_dw_dot_all_kernel, dim3((p.fin.max_cout + 63) / 64, (p.fin.max_krows + rpb - 1) / rpb, (unsigned)count), dim3(256), 0, st,
                       p.fin.tab + first, (const char*)p.ws, p.tr->params, p.tr->grads, rpb);
}
static void bn_grads(TrainPass& p, int first, int count, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(bn_param_grads_all_kernel, dim3((p.fin.max_cout + 127) / 128, (unsigned)count), dim3(128), 0, st, p.fin.tab + first,
                       (const char*)p.ws, p.tr->stats, p.net->desc.bn_eps, p.tr->grads);
}

// Finalisation table of every non-head layer, conv1 LAST (its weight gradient is the last launch of the pass: the other layers are
// finalised beside it); rebuilt (behind a stream synchronisation) when the plan's offsets change with the batch or the frame size
static int plan_finalisation(TrainPass& p) {
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; const dgp_net_desc& d = net->desc;
    if (!tr->d_fin_table || tr->fin_B != p.B || tr->fin_h != d.in_h || tr->fin_w != d.in_w) {      // offsets follow the plan
        std::vector<FinDesc> tab;
        tr->fin_of_layer.assign(net->layers.size(), -1);
        auto entry = [&](size_t li) {
            tr->fin_of_layer[li] = (int)tab.size();
            const ConvLayer& l = net->layers[li];
            const TLayer& t = tr->tl[li];
            FinDesc f{};
            f.dw_off = (long long)p.pl.dw_l[li]; f.cs_off = (long long)p.pl.cs_l[li];
            f.w_off = t.w_off; f.g_off = t.g_off; f.b_off = t.b_off; f.mean_off = t.mean_off; f.var_off = t.var_off;
            f.taps = l.KH * l.KW; f.cin = l.Cin; f.cin_real = t.cin_real; f.cout = l.Cout; f.d_scale = l.d_scale;
            tab.push_back(f);
        };
        for (size_t li = 0; li < net->layers.size(); ++li)
            if ((int)li != net->head_part && (int)li != net->head_locref && (int)li != net->conv1) entry(li);
        entry((size_t)net->conv1);
        if (!tr->d_fin_table) HIP_TRY(hipMalloc(&tr->d_fin_table, tab.size() * sizeof(FinDesc)));
        HIP_TRY(hipStreamSynchronize(p.s));        // (a previous pass may still read the old table)
        HIP_TRY(hipMemcpy(tr->d_fin_table, tab.data(), tab.size() * sizeof(FinDesc), hipMemcpyHostToDevice));
        tr->n_fin = (int)tab.size(); tr->fin_B = p.B; tr->fin_h = d.in_h; tr->fin_w = d.in_w;
    }
    p.fin.tab = reinterpret_cast<const FinDesc*>(tr->d_fin_table);
    for (size_t li = 0; li < net->layers.size(); ++li) {
        if ((int)li == net->head_part || (int)li == net->head_locref) continue;
        p.fin.max_cout = std::max(p.fin.max_cout, net->layers[li].Cout);
        p.fin.max_krows = std::max(p.fin.max_krows, net->layers[li].KH * net->layers[li].KW * tr->tl[li].cin_real);
    }
    return DGP_OK;
}

// Gradient groups (see dgp_trainer::GradGroup), built once per trainer after the finalisation table: cut the units, back to front, into
// runs of >= a quarter of the parameters each
static int plan_grad_groups(dgp_trainer* tr) {
    if (!tr->groups.empty()) return DGP_OK;
    const dgp_net* net = tr->net;
    const int nu = (int)net->units.size();
    auto layer_range = [&](int li, long long& lo, long long& hi) {
        if (li < 0) return;
        const ConvLayer& l = net->layers[li];
        const TLayer& t = tr->tl[li];
        const bool head = (li == net->head_part || li == net->head_locref);
        const long long wsz_ = head ? 9ll * (l.Cout / 4) * l.Cin : (long long)l.KH * l.KW * t.cin_real * l.Cout;
        const long long bsz_ = head ? l.Cout / 4 : l.Cout;
        auto acc = [&](long long off, long long n) { lo = std::min(lo, off); hi = std::max(hi, off + (n + 3) / 4 * 4); };
        acc(t.w_off, wsz_);
        if (!head) acc(t.g_off, bsz_);
        acc(t.b_off, bsz_);
    };
    std::vector<dgp_trainer::GradGroup> gs;
    dgp_trainer::GradGroup cur_g;
    long long lo = tr->n_train, hi = 0;
    int f_lo = tr->n_fin, f_n = 0;
    layer_range(net->head_part, lo, hi);
    layer_range(net->head_locref, lo, hi);
    for (int ui = nu - 1; ui >= 1; --ui) {
        const Unit& u = net->units[ui];
        for (int li : {u.sc, u.c1, u.c2, u.c3}) {
            if (li < 0) continue;
            layer_range(li, lo, hi);
            f_lo = std::min(f_lo, tr->fin_of_layer[li]); ++f_n;
        }
        if (hi - lo >= tr->n_train / 4 && gs.size() < 6) {
            cur_g.cut_ui = ui; cur_g.fin_first = f_lo; cur_g.fin_count = f_n; cur_g.lo = lo; cur_g.hi = hi;
            gs.push_back(cur_g);
            lo = tr->n_train; hi = 0; f_lo = tr->n_fin; f_n = 0;
        }
    }
    // the last group: everything in front of the last cut (its table rows are [0, first cut row) + the stem's row, finalised at the end)
    dgp_trainer::GradGroup last;
    last.cut_ui = -1; last.lo = 0; last.hi = gs.empty() ? tr->n_train : gs.back().lo;
    last.fin_first = 0; last.fin_count = gs.empty() ? tr->n_fin - 1 : gs.back().fin_first;
    bool ok = true;                              // the groups must tile the flat buffer and the table, back to front
    long long expect_hi = tr->n_train;
    int expect_f = tr->n_fin - 1;
    for (const auto& g : gs) {
        ok = ok && g.hi == expect_hi && g.fin_first + g.fin_count == expect_f && g.lo < g.hi;
        expect_hi = g.lo; expect_f = g.fin_first;
    }
    if (!ok) gs.clear(), last.hi = tr->n_train, last.fin_count = tr->n_fin - 1;
    gs.push_back(last);
    for (auto& g : gs)
        if (hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) return fail(DGP_ERR_HIP, "gradient groups: hipEventCreate failed");
    tr->groups = gs;
    return DGP_OK;
}

// a group is complete behind the weight gradients of its layers: finalise it on their stream and record its event
static hipError_t close_groups_at(TrainPass& p, int ui) {
    dgp_trainer* tr = p.tr;
    while (p.grp_next + 1 < tr->groups.size() && tr->groups[p.grp_next].cut_ui == ui) {
        auto& g = tr->groups[p.grp_next++];
        hipStream_t st = p.side.on ? p.ctx.s2 : p.s;
        finalise(p, g.fin_first, g.fin_count, st);
        bn_grads(p, g.fin_first, g.fin_count, st);
        hipError_t e2 = hipEventRecord(g.ev, st);
        if (e2 != hipSuccess) return e2;
    }
    return hipSuccess;
}

// H1 tensor `t` takes the range slot / predicted scale of the launch that wrote `src` (a converted copy of it)
static int adopt_h1(TrainPass& p, const void* t, const void* src) {
    RangeCtx& rng = p.ctx.rng;
    const float* slot = rng.of(src);
    const float* pv = rng.prev_of(slot);
    if (!slot || !pv) return fail(DGP_ERR_STATE, "16-bit tier: a gradient tensor has no predicted range");
    rng.set(t, slot);
    p.ctx.note_cells(t, pv);
    return DGP_OK;
}

// Both heads' parameter gradients of the 16-bit tier (the training step and the layer-level entry point dgp_heads_backward_h1): ONE
// weight-gradient launch over the merged H1 tensor (wc.d.Cout = CT columns: the part head's phases from column 0, the locref head's from
// column cpad0), then each head's finalisation from its own columns.
hipError_t heads_h1_param_grads(const WgradCall& wc, int njt0, int njt1, int cpad0, float* dw0, float* db0, float* dw1, float* db1, hipStream_t hs) {
    const int cin = wc.d.Cin, CT = wc.d.Cout;
    hipError_t e = wgrad_launch(wc, hs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(finalize_head_grads, dim3(grid_for(9ll * njt0 * cin)), dim3(256), 0, hs, wc.dwraw, wc.colsum, njt0, cin, CT, 0, dw0, db0);
    hipLaunchKernelGGL(finalize_head_grads, dim3(grid_for(9ll * njt1 * cin)), dim3(256), 0, hs, wc.dwraw, wc.colsum, njt1, cin, CT, cpad0, dw1, db1);
    return hipGetLastError();
}

// Heads of the 16-bit tier, both at once.  Their loss gradients are gathered into ONE H1 tensor (scale predicted from its range one
// step ago, slot_dph); ONE weight-gradient launch reads it and the H1 features in place (second stream), ONE H1 -> H1 data-gradient launch
// with the merged panel writes d features, gated by the features' ReLU, as the H1 tensor the last unit's backward reads.
static int backward_heads_h1(TrainPass& p, const float* dscmap, const float* dlocref, float* slot_dph) {
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; TrainCtx& ctx = p.ctx;
    const int B = p.B, fh = net->fh, fw = net->fw;
    const ConvLayer &l0 = net->layers[net->head_part], &l1 = net->layers[net->head_locref];
    const TLayer &t0 = tr->tl[net->head_part], &t1 = tr->tl[net->head_locref];
    const int CT = tr->hm_ct, njt0 = l0.Cout / 4, njt1 = l1.Cout / 4;
    float* const DPH = p.F(p.pl.dphh);
    const float* dprev = ctx.rng.prev_of(slot_dph);
    const float* featH = p.F(p.pl.xo[p.nu() - 1]);
    const auto fp = ctx.shadow_prev.find(featH);
    if (fp == ctx.shadow_prev.end()) return fail(DGP_ERR_STATE, "16-bit tier: the features have no predicted range");
    launch_head_gather_h1(dscmap, dlocref, B, fh, fw, njt0, t0.cpad, njt1, t1.cpad, CT, dprev, DPH, slot_dph, p.s);
    ctx.rng.set(DPH, slot_dph);
    ctx.note_cells(DPH, dprev);
    hipStream_t hs;
    if (int rc = p.side.fork(hs)) return rc;
    WgradCall wc = head_wgrad_call(B, fh, fw, l0.Cin, CT, p.F(p.pl.dwraw), p.F(p.pl.colsum));
    wc.x = {featH, ctx.rng.of(featH), featH, fp->second};
    wc.dy = {DPH, ctx.rng.of(DPH), DPH, dprev};
    wc.fail_flag = tr->d_fast_flag; wc.h1 = true;
    HIP_TRY(heads_h1_param_grads(wc, njt0, njt1, t0.cpad, tr->grads + t0.w_off, tr->grads + t0.b_off, tr->grads + t1.w_off, tr->grads + t1.b_off, hs));
    (void)ctx.rng.take();                    // (the slot the first head's launch takes in a plain pass: every pass takes its slots in one order)
    HIP_TRY(conv_launch(p, dgrad_call(wc.d, tr->d_hmT, tr->hm_nk, t0.cinP, DPH, p.GH[p.cur]).cells(2).gate(featH, 2), p.s));
    return DGP_OK;
}

// Heads on the parity path's kernels: per head gather the phases, parameter gradients, data gradient into G[cur] (the second head accumulates
// onto the first and gates by the last unit's ReLU).  feat: the fp32 features (a fast pass: the copy it left in feat32).
static int backward_heads_f32(TrainPass& p, const float* dscmap, const float* dlocref, float* slot_dph) {
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; const RangeCtx& rng = p.ctx.rng;
    const int B = p.B, fh = net->fh, fw = net->fw;
    float* const dwraw = p.F(p.pl.dwraw); float* const colsum = p.F(p.pl.colsum);
    float* const Gc = p.G[p.cur];
    const float* feat = p.fast ? p.F(p.pl.feat32) : p.F(p.pl.xo[p.nu() - 1]);
    // the per-head data-gradient panels (t.d_wT) are parity-only panels: a 16-bit pass that cannot merge its heads (DGP_TRAIN_HEADS_H1=0,
    // head widths the merged panel does not take) lands here after lazy syncs and must not read last step's weights
    if (tr->parity_stale)
        if (int rc = refresh_parity_panels(tr, p.s)) return rc;
    const size_t heads[2] = {(size_t)net->head_part, (size_t)net->head_locref};
    const float* dsrc[2] = {dscmap, dlocref};
    float* dph[2] = {p.F(p.pl.dph0), p.F(p.pl.dph1)};
    for (int k = 0; k < 2; ++k) {
        const ConvLayer& l = net->layers[heads[k]];
        const TLayer& t = tr->tl[heads[k]];
        const int njt = l.Cout / 4;
        const long long tot = (long long)B * fh * fw * t.cpad;
        hipLaunchKernelGGL(head_gather_kernel, dim3(grid_for(tot)), dim3(256), 0, p.s, dsrc[k], B, fh, fw, njt, t.cpad, dph[k], slot_dph);
        // the head's parameter gradients (fill + wgrad + finalise through the shared dwraw / colsum scratch, in stream order) go to the
        // second stream when the pass overlaps: the chain only needs dph[k] for the data gradient below
        hipStream_t hs;
        if (int rc = p.side.fork(hs)) return rc;
        WgradCall wc = head_wgrad_call(B, fh, fw, l.Cin, t.cpad, dwraw, colsum);
        wc.x = {feat, rng.of(feat)};
        wc.dy = {dph[k], rng.of(dph[k])};
        HIP_TRY(wgrad_launch(wc, hs));
        hipLaunchKernelGGL(finalize_head_grads, dim3(grid_for(9ll * njt * l.Cin)), dim3(256), 0, hs, dwraw, colsum, njt,
                           l.Cin, t.cpad, 0, tr->grads + t.w_off, tr->grads + t.b_off);
        // dfeat (+)= convT: 2x2 taps flipped, pad' = 0; second head accumulates onto the first; gate on the last
        HIP_TRY(conv_launch(p, dgrad_call(wc.d, t, dph[k], Gc).residual(k == 1 ? Gc : nullptr, 1, fh, fw).gate(k == 1 ? feat : nullptr), p.s));
    }
    return DGP_OK;
}

// the heads' data gradient in the form the last unit's backward reads
static int backward_heads_handover(TrainPass& p) {
    TrainCtx& ctx = p.ctx; const dgp_net* net = p.net;
    float* const Gc = p.G[p.cur];
    const long long n8 = (long long)p.B * net->fh * net->fw * net->units[p.nu() - 1].depth / 8;
    if (p.heads_h1) {
        // (the merged launch wrote the H1 tensor itself)
    } else if (p.h1p()) {
        // the heads' data gradient (fp32, from the kernels of the parity path) enters the H1 units as an H1 tensor
        float* const GHc = p.GH[p.cur];
        if (int rc = adopt_h1(p, GHc, Gc)) return rc;
        launch_f32_to_h1_pred(Gc, n8 * 8, ctx.shadow_prev[GHc], GHc, p.s);
    } else if (p.fast) {
        // the heads' data gradient came from a kernel that writes no fp16 copy, and the last unit's conv3 weight gradient can only read
        // its H2 activation through the LDS-DMA tile: make the copy here
        const float* pv = ctx.rng.prev_of(ctx.rng.of(Gc));
        const auto sb = ctx.shadow_base.find(Gc);
        if (!pv || sb == ctx.shadow_base.end()) return fail(DGP_ERR_STATE, "fast pass: no range for the heads' data gradient");
        launch_f32_to_shadow(Gc, n8, pv, sb->second, p.s);
        ctx.shadow_prev[Gc] = pv;
    }
    return DGP_OK;
}

// One bottleneck unit of the 16-bit tier: every tensor of this unit is an H1 tensor with a predicted scale; data gradients are H1 -> H1
// launches of the cell kernels (gate and residual read as H1), weight gradients read both operands in place (wgrad_dma_h1).
// GH[cur] = d loss / d (unit output), already gated by its ReLU.
static int backward_unit_h1(TrainPass& p, int ui) {
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; const TPlan& pl = p.pl; TrainCtx& ctx = p.ctx; hipStream_t s = p.s;
    const int B = p.B, ub = (int)p.ub;
    const Unit& u = net->units[ui];
    const int h = u.h, w = u.w, ho = u.ho, wo = u.wo;
    const float* xin = ui == 0 ? p.F(pl.pool) : p.F(pl.xo[ui - 1]);
    const ConvLayer &l1 = net->layers[u.c1], &l2 = net->layers[u.c2], &l3 = net->layers[u.c3];
    const TLayer &t1 = tr->tl[u.c1], &t2 = tr->tl[u.c2], &t3 = tr->tl[u.c3];
    float* const GoutH = p.GH[p.cur];
    float* const GinH = p.GH[p.cur ^ 1];
    float* const DR2H = p.F((ui & 1) ? pl.sh_dr2_b : pl.sh_dr2);
    float* const DR1H = p.F((ui & 1) ? pl.sh_dr1_b : pl.sh_dr1);
    float* const DXAH = p.F((ui & 1) ? pl.dxa_b : pl.dxa);
    const float* const R1 = p.F(pl.r1[ui]);
    const float* const R2 = p.F(pl.r2[ui]);
    const float* xinH = ui > ub ? xin : p.F(ui == 0 ? pl.sh_pool : pl.sh_xo[ui - 1]);       // (unit ub reads the H1 copy of its fp32 input)
    int rc;
    if ((rc = layer_param_grads(p, u.c3, {R2, ho, wo}, {GoutH, ho, wo}))) return rc;
    HIP_TRY(p.side.before_write(DR2H));
    HIP_TRY(conv_launch(p, dgrad_call(layer_desc(l3, B, ho, wo, ho, wo), t3, GoutH, DR2H).cells(2).gate(R2, 2), s));
    const int pb_h = u.pb_h, pb_w = u.pb_w;
    if ((rc = layer_param_grads(p, u.c2, {R1, h, w}, {DR2H, ho, wo}, u.stride, pb_h, pb_w))) return rc;
    const dgp_conv_desc fwd2 = layer_desc(l2, B, h, w, ho, wo, u.stride, pb_h, pb_w);
    HIP_TRY(p.side.before_write(DR1H));
    if (u.stride > 1) {
        // stride-2 conv2: its data gradient reads dR2 on the zero-stuffed grid (h1_zero_stuff)
        if (u.stride != 2) return fail(DGP_ERR_STATE, "16-bit tier: stride > 2");
        float* const ZS = p.F(pl.dr1);             // (the fp32 dR1 region is free while the H1 units run)
        const size_t zbytes = (size_t)B * 2 * ho * 2 * wo * l2.Cout * 2;
        if (zbytes > (size_t)4 * ((size_t)B * h * w * u.depth_bn)) return fail(DGP_ERR_STATE, "16-bit tier: zero-stuffed gradient does not fit");
        HIP_TRY(p.side.before_write(ZS));
        HIP_TRY(h1_zero_stuff(s, DR2H, B, ho, wo, l2.Cout, ZS));
        HIP_TRY(conv_launch(p, dgrad_call(fwd2, t2, ZS, DR1H, true).cells(2).gate(R1, 2).keys(DR2H, nullptr), s));
    } else {
        HIP_TRY(conv_launch(p, dgrad_call(fwd2, t2, DR2H, DR1H).cells(2).gate(R1, 2), s));
    }
    const float* dxa = GoutH;
    int dxa_mode = 1, dxa_h = ho, dxa_w = wo;
    if (u.sc >= 0) {
        if (u.stride != 1) return fail(DGP_ERR_STATE, "16-bit tier: strided shortcut conv");
        if ((rc = layer_param_grads(p, u.sc, {xin, h, w}, {GoutH, ho, wo}))) return rc;
        HIP_TRY(p.side.before_write(DXAH));
        HIP_TRY(conv_launch(p, dgrad_call(layer_desc(net->layers[u.sc], B, h, w, ho, wo), tr->tl[u.sc], GoutH, DXAH).cells(2), s));
        dxa = DXAH; dxa_h = h; dxa_w = w;
    } else if (u.stride > 1) {
        dxa_mode = -2;
    }
    if ((rc = layer_param_grads(p, u.c1, {xin, h, w}, {DR1H, h, w}))) return rc;
    HIP_TRY(p.side.before_write(GinH));
    HIP_TRY(conv_launch(p, dgrad_call(layer_desc(l1, B, h, w, h, w), t1, DR1H, GinH).residual(dxa, dxa_mode, dxa_h, dxa_w).cells(2, dxa).gate(xinH, 2), s));
    if (ui == ub && ub == 0 && p.stem_wgrad_h1) {
        // (unit 0's data gradient stays H1: the fused stem weight-gradient kernel reads it in place)
        p.stem_g = GinH;
        p.stem_g_prev = ctx.shadow_prev[GinH];
    } else if (ui == ub) {
        // the data gradient leaves the H1 units: fp32 copy for block1's kernels (same range slot: the epilogue tracked max |G| before rounding)
        float* Gf = p.G[p.cur ^ 1];
        HIP_TRY(p.side.before_write(Gf));
        const long long n8 = (long long)B * h * w * l1.Cin / 8;
        launch_h1_to_f32_pred(GinH, n8, ctx.shadow_prev[GinH], Gf, nullptr, s);
        ctx.rng.set(Gf, ctx.rng.of(GinH));
        ctx.shadow_prev.erase(Gf);
    }
    return DGP_OK;
}

// One bottleneck unit on the parity path's kernels (a fast H2 pass: the gates of units >= ub read the activations as H2 cells).
// G[cur] = d loss / d (unit output), already gated by its ReLU.
static int backward_unit_f32(TrainPass& p, int ui) {
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; const TPlan& pl = p.pl; hipStream_t s = p.s;
    const int B = p.B, ub = (int)p.ub;
    const Unit& u = net->units[ui];
    const int h = u.h, w = u.w, ho = u.ho, wo = u.wo;
    const float* xin = ui == 0 ? p.F(pl.pool) : p.F(pl.xo[ui - 1]);
    float* Gout = p.G[p.cur];
    float* Gin = p.G[p.cur ^ 1];
    const ConvLayer &l1 = net->layers[u.c1], &l2 = net->layers[u.c2], &l3 = net->layers[u.c3];
    const TLayer &t1 = tr->tl[u.c1], &t2 = tr->tl[u.c2], &t3 = tr->tl[u.c3];
    // gradient buffers of this unit (units alternate between two sets: a weight gradient still reading unit ui + 1's dR1 / dR2 on
    // the second stream does not hold this unit's chain back)
    float* const DR2 = p.F((ui & 1) ? pl.dr2_b : pl.dr2);
    float* const DR1 = p.F((ui & 1) ? pl.dr1_b : pl.dr1);
    float* const DXA = p.F((ui & 1) ? pl.dxa_b : pl.dxa);
    const float* const R1 = p.F(pl.r1[ui]);
    const float* const R2 = p.F(pl.r2[ui]);
    const int gate_fmt = (p.fast && ui >= ub) ? 1 : 0;     // this unit's activations are H2 tensors
    int rc;
    // conv3: params, then dR2 = convT(G) gated by R2 > 0; its copy feeds conv2's weight gradient (9 C1 x C1)
    if ((rc = layer_param_grads(p, u.c3, {R2, ho, wo}, {Gout, ho, wo}))) return rc;
    HIP_TRY(p.side.before_write(DR2));
    HIP_TRY(conv_launch(p, dgrad_call(layer_desc(l3, B, ho, wo, ho, wo), t3, Gout, DR2).gate(R2, gate_fmt).no_copy(u.depth_bn < 128), s));
    // conv2: params, then dR1 = convT(dR2) gated by R1 > 0; its copy feeds conv1's weight gradient (Cin x C1)
    const int pb_h = u.pb_h, pb_w = u.pb_w;
    if ((rc = layer_param_grads(p, u.c2, {R1, h, w}, {DR2, ho, wo}, u.stride, pb_h, pb_w))) return rc;
    HIP_TRY(p.side.before_write(DR1));
    HIP_TRY(conv_launch(p, dgrad_call(layer_desc(l2, B, h, w, ho, wo, u.stride, pb_h, pb_w), t2, DR2, DR1).gate(R1, gate_fmt)
                               .no_copy(!(u.depth_bn >= 128 && u.depth_in >= 128)), s));
    // shortcut branch
    const float* dxa = Gout;
    int dxa_mode = 1;                       // same grid
    int dxa_h = ho, dxa_w = wo;
    if (u.sc >= 0) {
        if ((rc = layer_param_grads(p, u.sc, {xin, h, w}, {Gout, ho, wo}, u.stride))) return rc;
        HIP_TRY(p.side.before_write(DXA));
        // (dXa is only added to the next data gradient: no copy)
        HIP_TRY(conv_launch(p, dgrad_call(layer_desc(net->layers[u.sc], B, h, w, ho, wo, u.stride), tr->tl[u.sc], Gout, DXA).no_copy(), s));
        dxa = DXA; dxa_h = h; dxa_w = w;
    } else if (u.stride > 1) {
        dxa_mode = -2;                      // subsample shortcut: gradient lives on the coarser grid
    }
    // conv1: params, then dX = (convT(dR1) + dXa) gated by X_in > 0  -> G for the previous unit (its copy feeds that unit's conv3 /
    // shortcut weight gradients; unit ub's input is block1's fp32 output)
    if ((rc = layer_param_grads(p, u.c1, {xin, h, w}, {DR1, h, w}))) return rc;
    HIP_TRY(p.side.before_write(Gin));       // (the G of two units ago: its conv3 / shortcut weight gradients)
    HIP_TRY(conv_launch(p, dgrad_call(layer_desc(l1, B, h, w, h, w), t1, DR1, Gin).residual(dxa, dxa_mode, dxa_h, dxa_w).gate(xin, (p.fast && ui > ub) ? 1 : 0)
                               .no_copy(!(ui > 0 && net->units[ui - 1].depth_bn >= 128)), s));
    return DGP_OK;
}

// Root block: max-pool backward (+ stem ReLU gate) and the stem's weight gradient -- or, 16-bit tier with the fused root block, both in
// stem_wgrad_h1_kernel reading unit 0's H1 data gradient.  The stem's weight gradient is the pass's last launch and nothing else is left to
// run beside it except the finalisation of all OTHER layers: that goes to the second stream behind the last of their weight gradients.
static int backward_root(TrainPass& p, bool fin_split) {
    dgp_trainer* tr = p.tr; const dgp_net* net = p.net; const TPlan& pl = p.pl; const dgp_net_desc& d = net->desc;
    const int B = p.B;
    hipStream_t s = p.s;
    if (p.stem_g) {
        if (fin_split) finalise(p, 0, tr->groups.back().fin_count, p.ctx.s2);      // (what the gradient groups have not finalised yet)
        StemWgradCall sa;
        sa.x = p.F(pl.p0); sa.g = p.stem_g; sa.idx = reinterpret_cast<const unsigned char*>(p.ws + pl.pidx);
        sa.g_prev = p.stem_g_prev;
        sa.dw = reinterpret_cast<float*>(p.ws + pl.dw_l[net->conv1]); sa.colsum = reinterpret_cast<float*>(p.ws + pl.cs_l[net->conv1]);
        sa.B = B; sa.H = d.in_h; sa.W = d.in_w; sa.H1 = net->h1; sa.W1 = net->w1; sa.HP = net->hp; sa.WP = net->wp;
        sa.slab = p.F(pl.dc1);               // (the d conv1 map's region: unused on this path; grid x 50 KB)
        stem_wgrad_launch(sa, s);
        return DGP_OK;
    }
    // (fused root block in the forward pass: no conv1 map -- unit 0's data gradient is already gated by pool > 0)
    launch_maxpool_bwd_idx((p.h1p() && tr->fwd_stem_fused) ? (const float*)nullptr : p.F(pl.c1), p.G[p.cur],
                           reinterpret_cast<const uchar4*>(p.ws + pl.pidx), B, net->h1, net->w1, net->hp, net->wp, p.F(pl.dc1), s);
    if (fin_split) finalise(p, 0, tr->groups.back().fin_count, p.ctx.s2);
    // (0.3 ms at 11 frames, fp32 MFMA on a 216 MB gradient; with the finalisation beside it: on the chain's stream)
    return layer_param_grads(p, net->conv1, {p.F(pl.p0), d.in_h, d.in_w}, {p.F(pl.dc1), net->h1, net->w1}, 2, 3, 3, !fin_split);
}

// End of the pass: the check of the 16-bit tier's predicted scales, the join, the last gradient group's finalisation
static int backward_finish(TrainPass& p, bool fin_split) {
    dgp_trainer* tr = p.tr; hipStream_t s = p.s;
    // every H1 gradient tensor of this pass against its predicted scale (wgrad_dma_h1 raised the same flag for its operands)
    if (p.h1p())
        if (int rc = check_predictions(p, "16-bit tier: too many H1 gradient tensors")) return rc;
    p.side.join();                               // every weight gradient has landed before the finalisation reads them
    const int rest = tr->groups.back().fin_count;      // rows [0, rest) + the stem's row: the last gradient group
    if (!fin_split) finalise(p, 0, rest, s);
    finalise(p, tr->n_fin - 1, 1, s);
    bn_grads(p, 0, rest, s);
    bn_grads(p, tr->n_fin - 1, 1, s);
    if (p.grp_next + 1 != tr->groups.size()) return fail(DGP_ERR_STATE, "backward: a gradient group was not closed");
    HIP_TRY(hipEventRecord(tr->groups.back().ev, s));
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

extern "C" int dgp_train_backward(dgp_trainer* tr, int32_t nt, void* workspace, size_t workspace_bytes, const float* dscmap,
                                  const float* dlocref, void* stream) {
    if (!tr || !workspace || !dscmap || !dlocref) return fail(DGP_ERR_INVALID, "dgp_train_backward: null argument");
    dgp_net* net = tr->net;
    const TPlan pl = make_tplan(tr, nt);
    if (workspace_bytes < pl.total) return fail(DGP_ERR_INVALID, "dgp_train_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    TrainPass p(tr, s, workspace, pl, nt);
    TrainCtx& ctx = p.ctx;
    range_pass_begin(tr, s, true);
    if (pl.sh_g0) {
        const size_t gb[6][2] = {{pl.g0, pl.sh_g0}, {pl.g1, pl.sh_g1}, {pl.dr1, pl.sh_dr1}, {pl.dr2, pl.sh_dr2}, {pl.dr1_b, pl.sh_dr1_b}, {pl.dr2_b, pl.sh_dr2_b}};
        for (const auto& q : gb) { ctx.shadow_base[p.F(q[0])] = p.F(q[1]); ctx.shadow_prev.erase(p.F(q[0])); }
    }
    HIP_TRY(hipMemsetAsync(p.ws + pl.dwall, 0, pl.dwall_bytes, s));
    // weight gradients on their own stream beside the data-gradient chain (DGP_WGRAD_OVERLAP=0: one stream, A/B)
    static const bool overlap_env = (dgp_tune("DGP_WGRAD_OVERLAP", 1) != 0);
    if (overlap_env) {
        if (int rc = ensure_side_stream(ctx)) return rc;
        p.side.begin(&ctx, s);
    }
    // what dgp_train_forward did: a fast pass left the activations of units >= ub as H2 tensors -- gates read them as such, weight gradients
    // read them in place, the heads use the fp32 copy in feat32; in the 16-bit tier the gradient tensors of those units are H1-only as well
    p.fast = tr->fwd_fast;
    p.fmt = p.fast ? tr->fwd_fmt : 1;
    p.ub = first_cell_unit(net, pl, p.h1p());
    if (p.h1p()) ctx.h2_slots.clear();                  // this pass's H1 gradient tensors, checked against their predicted scales at its end
    p.G[0] = p.F(pl.g0); p.G[1] = p.F(pl.g1);
    p.GH[0] = p.F(pl.sh_g0); p.GH[1] = p.F(pl.sh_g1);   // tier 1: G of the H1 units (the fp16-copy regions of the parity pass hold the tensors themselves)
    // range of the gathered loss gradients (both heads): the first slot of every backward pass -- it predicts the scale of the merged
    // H1 tensor of the next 16-bit pass
    float* const slot_dph = ctx.rng.take();
    p.heads_h1 = p.h1p() && tr->d_hmT && tr->d_hmT_h1 && slot_dph && ctx.rng.prev_of(slot_dph) && !tr->fwd_feat32;
    if (p.fast && !p.heads_h1 && !tr->fwd_feat32) return fail(DGP_ERR_STATE, "backward: the forward pass left no fp32 features for the heads");
    int rc = p.heads_h1 ? backward_heads_h1(p, dscmap, dlocref, slot_dph) : backward_heads_f32(p, dscmap, dlocref, slot_dph);
    if (rc || (rc = backward_heads_handover(p))) return rc;
    // 16-bit tier with the fused root block: the stem's weight gradient reads d pool as the H1 tensor unit 0 leaves (stem_wgrad_h1_kernel:
    // pool backward fused, no d conv1 map); A/B switch DGP_TRAIN_STEM_WGRAD_H1=0
    static const bool stem_wgrad_env = (dgp_tune("DGP_TRAIN_STEM_WGRAD_H1", 1) != 0);
    const ConvLayer& c1 = net->layers[net->conv1];
    p.stem_wgrad_h1 = stem_wgrad_env && p.h1p() && p.ub == 0 && tr->fwd_stem_fused && c1.Cout == 64 && c1.KH == 7 && c1.Cin == 4;
    if ((rc = plan_finalisation(p)) || (rc = plan_grad_groups(tr))) return rc;
    for (int ui = p.nu() - 1; ui >= 0; --ui) {
        rc = (p.h1p() && ui >= (int)p.ub) ? backward_unit_h1(p, ui) : backward_unit_f32(p, ui);
        if (rc) return rc;
        p.cur ^= 1;
        HIP_TRY(close_groups_at(p, ui));
    }
    const bool fin_split = p.side.on && tr->n_fin > 1;
    if ((rc = backward_root(p, fin_split))) return rc;
    return backward_finish(p, fin_split);
}

extern "C" {


/* Fast pass of the training step.  enable != 0: the NEXT dgp_train_forward keeps the retained activations of blocks 2-4 as H2 tensors
 * whose scales are predicted from the ranges the previous pass left behind (call it only after a pass of the same frame count and
 * size; the first pass after dgp_trainer_create, a weight upload or a shape change must be a plain one).  dgp_train_backward follows
 * what the forward did.  dgp_trainer_fast_status: call after the step's work has completed on the stream (it synchronises the
 * device); *failed != 0: a tensor left its predicted range, scoremaps and gradients of that step are NOT valid -- run the step again
 * with enable = 0 before using either. */
int dgp_trainer_fast_mode(dgp_trainer* tr, int32_t enable) {
    if (!tr) return fail(DGP_ERR_INVALID, "dgp_trainer_fast_mode: null");
#ifndef DGP_TUNING
    // (the H2 form measured no faster than the plain pass, EXPERIMENTS.md section 4: an opt-in of tuning builds only; the 16-bit tier's passes use it)
    if (enable && tr->tier != 1) return fail(DGP_ERR_INVALID, "dgp_trainer_fast_mode: needs dgp_trainer_set_tier(tr, 1) (the H2 fast pass is enabled in -DDGP_TUNING builds only)");
#endif
    tr->fast_next = enable != 0;
    return DGP_OK;
}
/* Gradient groups of the LAST dgp_train_backward (data-parallel training): group k = floats [lo[k], hi[k]) of the flat gradient buffer
 * (dgp_trainer_buffer(tr, 1)), in the order the pass completes them -- the heads and the last bottleneck units first, the stem last; the
 * groups tile the buffer.  *n_groups = 0 before the first backward pass. */
int dgp_trainer_grad_groups(dgp_trainer* tr, int32_t max_groups, int32_t* n_groups, int64_t* lo, int64_t* hi) {
    if (!tr || !n_groups) return fail(DGP_ERR_INVALID, "dgp_trainer_grad_groups: null");
    *n_groups = (int32_t)tr->groups.size();
    if ((int)tr->groups.size() > max_groups) return fail(DGP_ERR_INVALID, "dgp_trainer_grad_groups: more groups than max_groups");
    for (size_t k = 0; k < tr->groups.size(); ++k) {
        if (lo) lo[k] = tr->groups[k].lo;
        if (hi) hi[k] = tr->groups[k].hi;
    }
    return DGP_OK;
}
/* Makes `stream` wait until group k of the last dgp_train_backward is final in the gradient buffer (hipStreamWaitEvent: nothing blocks
 * on the host).  A communication stream that waits for group k can all-reduce it while the pass is still computing the later groups. */
int dgp_trainer_grad_group_wait(dgp_trainer* tr, int32_t k, void* stream) {
    if (!tr || k < 0 || k >= (int)tr->groups.size() || !tr->groups[k].ev) return fail(DGP_ERR_INVALID, "dgp_trainer_grad_group_wait: no such group");
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, tr->groups[k].ev, 0));
    return DGP_OK;
}
int dgp_trainer_set_tier(dgp_trainer* tr, int32_t tier) {
    if (!tr || (tier != 0 && tier != 1)) return fail(DGP_ERR_INVALID, "dgp_trainer_set_tier: tier must be 0 (parity) or 1 (16-bit)");
    tr->tier = tier;
    if (!tier) tr->fast_next = false;
    return DGP_OK;
}
int dgp_trainer_get_tier(const dgp_trainer* tr) { return tr ? tr->tier : 0; }

int dgp_trainer_fast_status(dgp_trainer* tr, int32_t* was_fast, int32_t* failed) {
    if (!tr || !failed) return fail(DGP_ERR_INVALID, "dgp_trainer_fast_status: null");
    int f = 0;
    if (tr->fwd_fast) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&f, tr->d_fast_flag, sizeof(int), hipMemcpyDeviceToHost));
    }
    if (was_fast) *was_fast = tr->fwd_fast ? 1 : 0;
    *failed = f;
    return DGP_OK;
}

}  // extern "C"
