// Weight (re)packing of the training step on the device, from the flat master parameter buffer: the pack kernels, the weight sync
// (dgp_trainer_sync_weights: master parameters -> forward panels, folded BN, data-gradient panels and their fp16 cells), the panels that
// only the parity path reads (refresh_parity_panels) and the data-gradient panel of the layer-level entry points (DgradPanel).
#include "dgp_train.h"

using namespace dgp;

namespace {

__device__ __forceinline__ float amax4(float m, const float4& v) {
    return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// head forward panels: W'[khp][kwp][ci][(a,b),c] = w[a+2-2khp][b+2-2kwp][c][ci] (w is [3,3,njt,Cin])
__global__ void pack_head_fwd_kernel(const float* __restrict__ w, int njt, int cin, int coutP, int nchunks,
                                     float* __restrict__ packed) {
    const long long total = (long long)nchunks * coutP;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(g % coutP);
        const int q = (int)(g / coutP);
        const int cin4 = cin >> 2;
        const int tap = q / cin4, ch = (q - tap * cin4) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tap < 4 && co < 4 * njt) {
            const int khp = tap >> 1, kwp = tap & 1, ph = co / njt, c = co - ph * njt;
            const int ka = (ph >> 1) + 2 - 2 * khp, kb = (ph & 1) + 2 - 2 * kwp;
            if (ka <= 2 && kb <= 2) {
                const float* src = w + (((long long)ka * 3 + kb) * njt + c) * cin + ch;
                v = make_float4(src[0], src[1], src[2], src[3]);
            }
        }
        *reinterpret_cast<float4*>(packed + g * 4) = v;
    }
}

// head weights as the pointwise panel of the engine's run_head_pointwise: row ci, column (tap, phase, joint) -> [2048 / 4][coutP][4];
// W'[khp][kwp][ci][(a,b),c] = w[a+2-2khp][b+2-2kwp][c][ci] (w is [3,3,njt,Cin]); tracks max |panel| for the fp16 cells
__global__ void pack_head_pw_kernel(const float* __restrict__ w, int njt, int cin, int coutP, float* __restrict__ packed,
                                    float* __restrict__ rng) {
    float mx = 0.f;
    const long long total = (long long)(cin >> 2) * coutP;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int col = (int)(g % coutP);
        const int ch = (int)(g / coutP) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < 16 * njt) {
            const int tap = col / (4 * njt), r = col - tap * 4 * njt, ph = r / njt, c = r - ph * njt;
            const int khp = tap >> 1, kwp = tap & 1;
            const int ka = (ph >> 1) + 2 - 2 * khp, kb = (ph & 1) + 2 - 2 * kwp;
            if (ka <= 2 && kb <= 2) {
                const float* src = w + (((long long)ka * 3 + kb) * njt + c) * cin + ch;
                v = make_float4(src[0], src[1], src[2], src[3]);
            }
        }
        *reinterpret_cast<float4*>(packed + g * 4) = v;
        mx = amax4(mx, v);
    }
    pack_track(rng, mx);
}

__global__ void head_bias_kernel(const float* __restrict__ b, int njt, float* __restrict__ bias4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * njt) bias4[i] = b[i % njt];
}

// data-gradient panels: Wd[tap'][co][ci] = W[taps-1-tap'][ci][co] * scale[co]; K' = taps*Cout (co fastest), N' = Cin
__global__ void pack_dgrad_kernel(const float* __restrict__ w, const float* __restrict__ scale, int taps, int cin,
                                  int cout, int cinP, int nchunks, float* __restrict__ packed, float* __restrict__ rng) {
    float mx = 0.f;
    const long long total = (long long)nchunks * cinP;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(g % cinP);
        const int q = (int)(g / cinP);
        const int cout4 = cout >> 2;
        const int tapp = q / cout4, co = (q - tapp * cout4) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tapp < taps && ci < cin) {
            const int tap = taps - 1 - tapp;          // spatial flip (row-major taps: flipping both axes reverses the index)
            const float* src = w + ((long long)tap * cin + ci) * cout + co;
            v = make_float4(src[0] * scale[co], src[1] * scale[co + 1], src[2] * scale[co + 2], src[3] * scale[co + 3]);
        }
        *reinterpret_cast<float4*>(packed + g * 4) = v;
        mx = amax4(mx, v);
    }
    pack_track(rng, mx);
}

// All non-head layers in ONE launch (a launch per layer and job costs ~180 dispatches of 4 us + their gaps per step):
// blockIdx.y = layer, blockIdx.z = job (0: forward panel [nk*8][CoutP][4] from HWIO [KH*KW][Cin_real][Cout], 1: data-gradient panel
// as pack_dgrad_kernel lays it out, 2: folded BN: scale = gamma / sqrtf(var + eps), bias = beta - mean * scale).  The data-gradient
// job evaluates the same expression for scale itself (so the same bits) instead of waiting for job 2.  (PackDesc: dgp_train.h)
__global__ __launch_bounds__(256) void pack_all_kernel(const PackDesc* __restrict__ table, const float* __restrict__ params,
                                                       const float* __restrict__ stats, float eps) {
    const PackDesc d = table[blockIdx.y];
    const float* w = params + d.w_off;
    if (blockIdx.z == 2) {
        for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < d.cout; c += gridDim.x * blockDim.x) {
            const float inv = params[d.g_off + c] / sqrtf(stats[d.var_off + c] + eps);
            d.d_scale[c] = inv;
            d.d_bias[c] = params[d.b_off + c] - stats[d.mean_off + c] * inv;
        }
        return;
    }
    float mx = 0.f;
    if (blockIdx.z == 0) {
        const long long total = (long long)d.nchunks_f * d.coutP;
        if ((long long)blockIdx.x * blockDim.x >= total) return;
        const int cin4 = d.cin >> 2;
        for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
            const int co = (int)(g % d.coutP);
            const int q = (int)(g / d.coutP);
            const int tap = q / cin4, ch = (q - tap * cin4) << 2;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tap < d.taps && co < d.cout) {
                float* pv = &v.x;
                for (int e = 0; e < 4; ++e)
                    if (ch + e < d.cin_real) pv[e] = w[((long long)tap * d.cin_real + ch + e) * d.cout + co];
            }
            *reinterpret_cast<float4*>(d.d_w + g * 4) = v;
            mx = amax4(mx, v);
        }
        pack_track(d.rng_f, mx);
    } else {
        if (!d.d_wT) return;
        const long long total = (long long)d.nchunks_b * d.cinP;
        if ((long long)blockIdx.x * blockDim.x >= total) return;
        const int cout4 = d.cout >> 2;
        for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
            const int ci = (int)(g % d.cinP);
            const int q = (int)(g / d.cinP);
            const int tapp = q / cout4, co = (q - tapp * cout4) << 2;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tapp < d.taps && ci < d.cin) {
                const int tap = d.taps - 1 - tapp;
                const float* src = w + ((long long)tap * d.cin + ci) * d.cout + co;
                float sc[4];
                for (int e = 0; e < 4; ++e) sc[e] = params[d.g_off + co + e] / sqrtf(stats[d.var_off + co + e] + eps);
                v = make_float4(src[0] * sc[0], src[1] * sc[1], src[2] * sc[2], src[3] * sc[3]);
            }
            *reinterpret_cast<float4*>(d.d_wT + g * 4) = v;
            mx = amax4(mx, v);
        }
        pack_track(d.rng_b, mx);
    }
}

// head data-gradient panels: "input" channels = phase-major 4*njt padded to cpad, taps 2x2 flipped, N' = Cin
__global__ void pack_head_dgrad_kernel(const float* __restrict__ w, int njt, int cin, int cpad, int cinP, int nchunks,
                                       float* __restrict__ packed) {
    const long long total = (long long)nchunks * cinP;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(g % cinP);
        const int q = (int)(g / cinP);
        const int c4 = cpad >> 2;
        const int tapp = q / c4, cob = (q - tapp * c4) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tapp < 4 && ci < cin) {
            const int tap = 3 - tapp, khp = tap >> 1, kwp = tap & 1;
            float* pv = &v.x;
            for (int e = 0; e < 4; ++e) {
                const int co = cob + e;
                if (co >= 4 * njt) continue;
                const int ph = co / njt, c = co - ph * njt;
                const int ka = (ph >> 1) + 2 - 2 * khp, kb = (ph & 1) + 2 - 2 * kwp;
                if (ka <= 2 && kb <= 2) pv[e] = w[(((long long)ka * 3 + kb) * njt + c) * cin + ci];
            }
        }
        *reinterpret_cast<float4*>(packed + g * 4) = v;
    }
}

// 16-bit tier: BOTH heads' data-gradient panels side by side -- "input" channels [0, cpad0) the part head's phases, [cpad0, cpad0 +
// cpad1) the locref head's, zero up to CT -- so that one launch over head_gather_h1_kernel's tensor gives d features of both heads
__global__ void pack_heads_dgrad_kernel(const float* __restrict__ w0, int njt0, int cpad0, const float* __restrict__ w1, int njt1, int cpad1,
                                        int cin, int CT, int cinP, int nchunks, float* __restrict__ packed, float* __restrict__ rng) {
    const long long total = (long long)nchunks * cinP;
    float mx = 0.f;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(g % cinP);
        const int q = (int)(g / cinP);
        const int c4 = CT >> 2;
        const int tapp = q / c4, cob = (q - tapp * c4) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tapp < 4 && ci < cin) {
            const int tap = 3 - tapp, khp = tap >> 1, kwp = tap & 1;
            float* pv = &v.x;
            for (int e = 0; e < 4; ++e) {
                int co = cob + e;
                const float* w = w0;
                int njt = njt0;
                if (co >= cpad0) { co -= cpad0; w = w1; njt = njt1; if (co >= cpad1) continue; }
                if (co >= 4 * njt) continue;
                const int ph = co / njt, c = co - ph * njt;
                const int ka = (ph >> 1) + 2 - 2 * khp, kb = (ph & 1) + 2 - 2 * kwp;
                if (ka <= 2 && kb <= 2) pv[e] = w[(((long long)ka * 3 + kb) * njt + c) * cin + ci];
            }
        }
        *reinterpret_cast<float4*>(packed + g * 4) = v;
        mx = amax4(mx, v);
    }
    pack_track(rng, mx);
}

// Stem panel [49 taps][CoutP][4] -> the row panel of the fused root kernel [7 kernel rows x 8 pixels][CoutP][4]: pixel 7 is zero, and channel
// slot 3 carries sum_c (round(mean_c) - mean_c) w_c, the weight of the kernel's constant fourth input channel (dgp_net_load_weights builds
// the same panel on the host, dgp_net.hip).
__global__ __launch_bounds__(256) void stem_rows_kernel(const float4* __restrict__ panel, int coutP, float d0, float d1, float d2,
                                                        float4* __restrict__ rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 56 * coutP) return;
    const int r = i / coutP, co = i - r * coutP;
    const int kh = r >> 3, kw = r & 7;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kw < 7) {
        v = panel[(size_t)(kh * 7 + kw) * coutP + co];
        v.w = d0 * v.x + d1 * v.y + d2 * v.z;
    }
    rows[i] = v;
}

}  // namespace

void launch_pack_all(const void* table_dev, int n_layers, int n_jobs, const float* params, const float* stats, float eps, hipStream_t s) {
    hipLaunchKernelGGL(pack_all_kernel, dim3(256, (unsigned)n_layers, (unsigned)n_jobs), dim3(256), 0, s,
                       reinterpret_cast<const PackDesc*>(table_dev), params, stats, eps);
}

void launch_pack_heads_dgrad(const float* w0, int njt0, int cpad0, const float* w1, int njt1, int cpad1, int cin, int CT, int cinP, int nkT,
                             float* packed, float* rng, hipStream_t s) {
    hipLaunchKernelGGL(pack_heads_dgrad_kernel, dim3(grid_for((long long)nkT * 8 * cinP)), dim3(256), 0, s, w0, njt0, cpad0, w1, njt1, cpad1, cin,
                       CT, cinP, nkT * 8, packed, rng);
}

DgradPanel::DgradPanel(const dgp_conv_desc& d, void* scratch) : nkT(nk_for(d.KH, d.KW, d.Cout)), cinP(coutp_for(d.Cin)) {
    const size_t panel_bytes = (size_t)nkT * 8 * cinP * 16;
    char* const base = (char*)scratch;
    size_t o = 0;
    auto take = [&](size_t b) { char* q = base ? base + o : nullptr; o += b; return q; };
    panel = (float*)take(panel_bytes);
    cells = take(panel_bytes);
    rng = (float*)take(4 * ABSMAX_SLOTS * sizeof(float));
    ones = (float*)take((size_t)d.Cout * sizeof(float));
    bytes = o + 1024;
}

int DgradPanel::pack(const dgp_conv_desc& d, const float* w_hwio, const float* scale, hipStream_t s) const {
    HIP_TRY(hipMemsetAsync(rng, 0, 4 * ABSMAX_SLOTS * sizeof(float), s));
    if (!scale) {
        std::vector<float> h(d.Cout, 1.f);
        HIP_TRY(hipMemcpyAsync(ones, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        scale = ones;
    }
    hipLaunchKernelGGL(pack_dgrad_kernel, dim3(grid_for((long long)nkT * 8 * cinP)), dim3(256), 0, s, w_hwio, scale, d.KH * d.KW, d.Cin, d.Cout,
                       cinP, nkT * 8, panel, rng + ABSMAX_SLOTS);
    return DGP_OK;
}

// the heads' panels that only the parity path reads + the H2 cells of all panels, from the current master parameters / fp32 panels
int refresh_parity_panels(dgp_trainer* tr, hipStream_t s) {
    dgp_net* net = tr->net;
    for (int hd : {net->head_part, net->head_locref}) {
        ConvLayer& l = net->layers[hd];
        TLayer& t = tr->tl[hd];
        const float* w = tr->params + t.w_off;
        const int njt = l.Cout / 4;
        hipLaunchKernelGGL(pack_head_fwd_kernel, dim3(grid_for((long long)l.nk * 8 * l.CoutP)), dim3(256), 0, s, w, njt, l.Cin, l.CoutP, l.nk * 8, l.d_w);
        hipLaunchKernelGGL(pack_head_dgrad_kernel, dim3(grid_for((long long)t.nkT * 8 * t.cinP)), dim3(256), 0, s, w, njt, l.Cin, t.cpad, t.cinP,
                           t.nkT * 8, t.d_wT);
    }
    if (tr->d_h3_table) HIP_TRY(launch_pack_h3_all(reinterpret_cast<const PackH3Desc*>(tr->d_h3_table), tr->n_h3, s));
    HIP_TRY(hipGetLastError());
    tr->parity_stale = false;
    return DGP_OK;
}

// dgp_net::owner_sync: a forward on the trainer's net (Trainer.net.infer between steps) reads the heads' 2x2-conv panels and the H2 cells,
// which a 16-bit trainer leaves stale between plain passes
int trainer_owner_sync(void* owner, void* stream) {
    dgp_trainer* tr = static_cast<dgp_trainer*>(owner);
    if (!tr || !tr->parity_stale) return DGP_OK;
    return refresh_parity_panels(tr, (hipStream_t)stream);
}

// The fused root block's weight cells (stem_pool_fused_kernel) from conv1's forward panel [49 taps][CoutP][4]: the row panel
// [7 kernel rows x 8 pixels][CoutP][4] whose fourth channel slot carries the fraction of the mean pixel, then its fp16 high / low cells
// split with the PANEL's range slots.  rows / cells: 56 * CoutP * 4 floats each.  (The weight sync and dgp_root_block.)
hipError_t build_stem_cells(const float* panel, int CoutP, const float* mean_pixel, const float* panel_rng, float* rows, void* cells,
                            hipStream_t s) {
    hipLaunchKernelGGL(stem_rows_kernel, dim3((56 * CoutP + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4*>(panel), CoutP,
                       roundf(mean_pixel[0]) - mean_pixel[0], roundf(mean_pixel[1]) - mean_pixel[1], roundf(mean_pixel[2]) - mean_pixel[2],
                       reinterpret_cast<float4*>(rows));
    return launch_pack_h3(rows, 7, CoutP, panel_rng, cells, s);
}

extern "C" {

// master parameters -> forward panels / folded BN / data-gradient panels of the engine
int dgp_trainer_sync_weights(dgp_trainer* tr, void* stream) {
    if (!tr) return fail(DGP_ERR_INVALID, "dgp_trainer_sync_weights: null");
    dgp_net* net = tr->net;
    hipStream_t s = (hipStream_t)stream;
    const float eps = net->desc.bn_eps;
    const size_t nl_all = net->layers.size();
    if (tr->d_wrng) HIP_TRY(hipMemsetAsync(tr->d_wrng, 0, 2 * nl_all * ABSMAX_SLOTS * sizeof(float), s));
    // tier 1, every sync after the first: the parity-only panels wait for a plain pass
    const bool lazy = g_train_cells && tr->tier == 1 && tr->d_h3_table && tr->d_h1_table && tr->d_wrng;
    tr->parity_stale = lazy;
    for (ConvLayer& l : net->layers) {
        if (!l.d_w) HIP_TRY(hipMalloc(&l.d_w, (size_t)l.nk * 8 * l.CoutP * 4 * sizeof(float)));
        if (!l.d_scale) HIP_TRY(hipMalloc(&l.d_scale, l.Cout * sizeof(float)));
        if (!l.d_bias) HIP_TRY(hipMalloc(&l.d_bias, l.Cout * sizeof(float)));
    }
    for (int hd : {net->head_part, net->head_locref}) {
        ConvLayer& l = net->layers[hd];
        TLayer& t = tr->tl[hd];
        float* rng_f = tr->d_wrng ? tr->d_wrng + (size_t)hd * ABSMAX_SLOTS : nullptr;          // range of the pointwise panel packed below
        const float* w = tr->params + t.w_off;
        const long long tot = (long long)l.nk * 8 * l.CoutP;
        const int njt = l.Cout / 4;
        if (!lazy) hipLaunchKernelGGL(pack_head_fwd_kernel, dim3(grid_for(tot)), dim3(256), 0, s, w, njt, l.Cin, l.CoutP, l.nk * 8, l.d_w);
        if (g_train_cells && rng_f) {      // pointwise form of the same head for the forward pass (cells built below)
            l.coutp_pw = head_pw_coutp(16 * njt);      // same width as dgp_net_load_weights gives the shared buffers
            const size_t npw = (size_t)nk_for(1, 1, l.Cin) * 8 * l.coutp_pw * 4;
            if (!l.d_w_pw) HIP_TRY(hipMalloc(&l.d_w_pw, npw * sizeof(float)));
            if (!l.d_wh3_pw) HIP_TRY(hipMalloc(&l.d_wh3_pw, npw * sizeof(float)));
            hipLaunchKernelGGL(pack_head_pw_kernel, dim3(grid_for((long long)(l.Cin >> 2) * l.coutp_pw)), dim3(256), 0, s, w, njt,
                               l.Cin, l.coutp_pw, l.d_w_pw, rng_f);
        }
        hipLaunchKernelGGL(head_bias_kernel, dim3(1), dim3(256), 0, s, tr->params + t.b_off, njt, l.d_bias);
        const long long totT = (long long)t.nkT * 8 * t.cinP;
        if (!lazy) hipLaunchKernelGGL(pack_head_dgrad_kernel, dim3(grid_for(totT)), dim3(256), 0, s, w, njt, l.Cin, t.cpad, t.cinP,
                                      t.nkT * 8, t.d_wT);
    }
    // one launch for the panels / folded BN of all non-head layers
    if (!tr->d_pack_table) {
        std::vector<PackDesc> tab;
        for (size_t li = 0; li < net->layers.size(); ++li) {
            if ((int)li == net->head_part || (int)li == net->head_locref) continue;
            const ConvLayer& l = net->layers[li];
            const TLayer& t = tr->tl[li];
            PackDesc d{};
            d.w_off = t.w_off; d.g_off = t.g_off; d.b_off = t.b_off; d.mean_off = t.mean_off; d.var_off = t.var_off;
            d.taps = l.KH * l.KW; d.cin_real = t.cin_real; d.cin = l.Cin; d.cout = l.Cout; d.coutP = l.CoutP;
            d.nchunks_f = l.nk * 8; d.cinP = t.cinP; d.nchunks_b = t.nkT * 8;
            d.d_w = l.d_w; d.rng_f = tr->d_wrng ? tr->d_wrng + li * ABSMAX_SLOTS : nullptr;
            d.d_wT = t.d_wT; d.rng_b = tr->d_wrng ? tr->d_wrng + (nl_all + li) * ABSMAX_SLOTS : nullptr;
            d.d_scale = l.d_scale; d.d_bias = l.d_bias;
            tab.push_back(d);
        }
        tr->n_pack = (int)tab.size();
        HIP_TRY(hipMalloc(&tr->d_pack_table, tab.size() * sizeof(PackDesc)));
        HIP_TRY(hipMemcpy(tr->d_pack_table, tab.data(), tab.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
    }
    launch_pack_all(tr->d_pack_table, tr->n_pack, 3, tr->params, tr->stats, eps, s);
    if (g_train_cells && tr->d_wrng) {        // the panels' fp16 cells, split with the ranges the launch above has just tracked
        // The table of one cell format (`bytes` of cells per float4 of panel): per non-head layer the forward panel, then the data-gradient
        // panel, each where takes(K, nk, NP) holds, then the heads' pointwise panels (range slot of the layer).  fwd / bwd / pw: the member
        // that owns a panel's cells, allocated here; reg(panel, cells) enters a non-head panel's cells into the trainer's lookup.
        auto cell_table = [&](int bytes, auto takes, void* ConvLayer::*fwd, void* TLayer::*bwd, void* ConvLayer::*pw, auto reg, void** d_table,
                              int* n) -> int {
            std::vector<PackH3Desc> tab;
            for (size_t li = 0; li < net->layers.size(); ++li) {
                if ((int)li == net->head_part || (int)li == net->head_locref) continue;
                ConvLayer& l = net->layers[li];
                TLayer& t = tr->tl[li];
                if (takes(l.Cin, l.nk, l.CoutP)) {
                    if (!(l.*fwd)) HIP_TRY(hipMalloc(&(l.*fwd), (size_t)l.nk * 8 * l.CoutP * bytes));
                    tab.push_back(PackH3Desc{l.d_w, l.nk * 4, l.CoutP, tr->d_wrng + li * ABSMAX_SLOTS, l.*fwd});
                    reg(l.d_w, l.*fwd);
                }
                if (t.d_wT && takes(l.Cout, t.nkT, t.cinP)) {
                    if (!(t.*bwd)) HIP_TRY(hipMalloc(&(t.*bwd), (size_t)t.nkT * 8 * t.cinP * bytes));
                    tab.push_back(PackH3Desc{t.d_wT, t.nkT * 4, t.cinP, tr->d_wrng + (nl_all + li) * ABSMAX_SLOTS, t.*bwd});
                    reg(t.d_wT, t.*bwd);
                }
            }
            for (int hd : {net->head_part, net->head_locref}) {
                ConvLayer& l = net->layers[hd];
                if (!l.d_w_pw) continue;
                const int nk = nk_for(1, 1, l.Cin);
                if (!(l.*pw)) HIP_TRY(hipMalloc(&(l.*pw), (size_t)nk * 8 * l.coutp_pw * bytes));
                tab.push_back(PackH3Desc{l.d_w_pw, nk * 4, l.coutp_pw, tr->d_wrng + (size_t)hd * ABSMAX_SLOTS, l.*pw});
            }
            *n = (int)tab.size();
            HIP_TRY(hipMalloc(d_table, tab.size() * sizeof(PackH3Desc)));
            HIP_TRY(hipMemcpy(*d_table, tab.data(), tab.size() * sizeof(PackH3Desc), hipMemcpyHostToDevice));
            return DGP_OK;
        };
        int rc;
        if (!tr->d_h3_table &&
            (rc = cell_table(16, [](int K, int, int) { return K >= 32; }, &ConvLayer::d_wh3, &TLayer::d_wTh3, &ConvLayer::d_wh3_pw,
                             [&](const float* panel, void* c) { tr->ctx.cells[panel] = static_cast<const float*>(c); }, &tr->d_h3_table, &tr->n_h3)))
            return rc;
        if (!lazy) HIP_TRY(launch_pack_h3_all(reinterpret_cast<const PackH3Desc*>(tr->d_h3_table), tr->n_h3, s));
        if (tr->tier == 1) {              // 16-bit tier: the same panels as high-only H1 cells (K-steps of 64 channels: K % 64 == 0)
            if (!tr->d_h1_table &&
                (rc = cell_table(8, [](int K, int nk, int NP) { return K >= 64 && K % 64 == 0 && nk % 2 == 0 && NP % 64 == 0; }, &ConvLayer::d_wh1,
                                 &TLayer::d_wTh1, &ConvLayer::d_wh1_pw, [&](const float* panel, void* c) { tr->ctx.cells1[panel] = c; },
                                 &tr->d_h1_table, &tr->n_h1)))
                return rc;
            HIP_TRY(launch_pack_h1_all(reinterpret_cast<const PackH3Desc*>(tr->d_h1_table), tr->n_h1, s));
            // both heads' data-gradient panels as one panel + its H1 cells (one launch gives d features of both heads)
            static const bool heads_h1_env = (dgp_env("DGP_TRAIN_HEADS_H1", 1) != 0);      // A/B switch
            {
                const ConvLayer &l0 = net->layers[net->head_part], &l1 = net->layers[net->head_locref];
                const TLayer &t0 = tr->tl[net->head_part], &t1 = tr->tl[net->head_locref];
                const int CT = heads_ct(net->desc.num_joints), nkT = nk_for(2, 2, CT);
                if (heads_h1_env && l0.Cin == l1.Cin && t0.cinP == t1.cinP && t0.cpad + t1.cpad <= CT && (nkT % 2) == 0 && t0.cinP % 64 == 0) {
                    const size_t pbytes = (size_t)nkT * 8 * t0.cinP * 16;
                    if (!tr->d_hmT) HIP_TRY(hipMalloc(&tr->d_hmT, pbytes));
                    if (!tr->d_hmT_h1) HIP_TRY(hipMalloc(&tr->d_hmT_h1, pbytes / 2));
                    if (!tr->d_hm_rng) HIP_TRY(hipMalloc(&tr->d_hm_rng, ABSMAX_SLOTS * sizeof(float)));
                    tr->hm_ct = CT; tr->hm_nk = nkT;
                    HIP_TRY(hipMemsetAsync(tr->d_hm_rng, 0, ABSMAX_SLOTS * sizeof(float), s));
                    launch_pack_heads_dgrad(tr->params + t0.w_off, l0.Cout / 4, t0.cpad, tr->params + t1.w_off, l1.Cout / 4, t1.cpad, l0.Cin, CT,
                                            t0.cinP, nkT, tr->d_hmT, tr->d_hm_rng, s);
                    HIP_TRY(launch_pack_h1(tr->d_hmT, nkT, t0.cinP, tr->d_hm_rng, tr->d_hmT_h1, s));
                    tr->ctx.cells1[tr->d_hmT] = tr->d_hmT_h1;
                }
            }
            // the fused root block's weight cells (stem_pool_fused_kernel): row panel of conv1 from the panel pack_all_kernel just wrote
            static const bool stem_fused_env = (dgp_tune("DGP_TRAIN_STEM_FUSED", 1) != 0);      // A/B switch
            ConvLayer& lc = net->layers[net->conv1];
            if (stem_fused_env && lc.CoutP == 64 && lc.Cin == 4 && lc.KH == 7 && lc.KW == 7) {
                const size_t nrow = (size_t)56 * lc.CoutP * 4;
                if (!tr->d_stem_rows) HIP_TRY(hipMalloc(&tr->d_stem_rows, nrow * sizeof(float)));
                if (!tr->d_stem_cells) HIP_TRY(hipMalloc(&tr->d_stem_cells, nrow * sizeof(float)));
                HIP_TRY(build_stem_cells(lc.d_w, lc.CoutP, net->desc.mean_pixel, tr->d_wrng + (size_t)net->conv1 * ABSMAX_SLOTS, tr->d_stem_rows,
                                         tr->d_stem_cells, s));
            }
        }
    }
    HIP_TRY(hipGetLastError());
    net->wmax_valid = false;      // panels changed: weight ranges of the fp16-split kernels are stale
    net->loaded = true;
    return DGP_OK;
}

}  // extern "C"
