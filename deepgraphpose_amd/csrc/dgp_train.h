// Trainer-internal types and launchers shared by the files of the training step: dgp_train.hip (the trainer and its passes),
// dgp_wgrad.hip (weight-gradient kernels), dgp_train_pack.hip (weight re-packing and the weight sync), dgp_optim.hip (optimisers, step
// status) and dgp_train_layers.hip (the layer-level entry points of tests and sweep scripts).  No relocatable device code: a kernel lives in
// the file that launches it, and a kernel that two files need has ONE host launcher in its file, declared here.
#pragma once
#include "dgp_engine.h"

#include <algorithm>
#include <unordered_map>

inline int grid_for(long long n) {
    long long b = (n + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
inline int next_pow2(int x) { int p = 4; while (p < x) p <<= 1; return p; }
// channels of the merged heads tensor: both heads' padded phase columns, rounded up to the H1 kernels' K-step
inline int heads_ct(int nj) { return (next_pow2(4 * nj) + next_pow2(8 * nj) + 63) / 64 * 64; }

// Kernel arguments and device helpers of kernels in unnamed namespaces (every file sees its own copy of the type, as the kernels' names want)
namespace {

// max |v| of what a pack kernel wrote -> the panel's range slots (fp16-split convs of the training step); non-negative floats
// order like their bit patterns, slots spread the atomics
__device__ __forceinline__ void pack_track(float* rng, float m) {
    if (!rng) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0)
        atomicMax(reinterpret_cast<unsigned*>(rng) + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (dgp::ABSMAX_SLOTS - 1)), __float_as_uint(m));
}

// one non-head layer of pack_all_kernel's table (dgp_train_pack.hip)
struct PackDesc {
    long long w_off, g_off, b_off, mean_off, var_off;
    int taps, cin_real, cin, cout, coutP, nchunks_f, cinP, nchunks_b;
    float *d_w, *rng_f, *d_wT, *rng_b, *d_scale, *d_bias;
};

}  // namespace

// ================================================================================================
// trainer
// ================================================================================================
struct TLayer {
    long long w_off = -1, g_off = -1, b_off = -1;     // offsets into the flat trainable buffer (floats)
    long long mean_off = -1, var_off = -1;            // offsets into the frozen-statistics buffer
    int cin_real = 0;
    float* d_wT = nullptr;                            // data-gradient panels
    void* d_wTh3 = nullptr;                           // ... pre-split into fp16 high/low cells (launch_pack_h3), per sync
    void* d_wTh1 = nullptr;                           // ... as high-only H1 cells (tier 1)
    int nkT = 0, cinP = 0, cpad = 0;                  // cpad: padded phase-major channel count (heads)
};

// Operand ranges for the fp16-split conv kernels inside the training step.  Every conv launched through conv_launch takes a
// fresh slot array from a pool for max |out| and records it under its output pointer; a later conv whose input pointer (and
// weight panel) has a recorded range runs the fp16 kernels, anything else (tensors written by other kernels: pooling, loss
// gradients, head gathers) falls back to the range-free bf16 split.  The pool is zeroed at the start of each pass.
constexpr int RANGE_POOL = 768;             // forward chain 1 [0, 256) | forward chain 2 [256, 512) | backward [512, 768)
constexpr int RANGE_FWD = 256;

struct RangeCtx {
    float* pool = nullptr;            // RANGE_POOL slot arrays of ABSMAX_SLOTS floats
    float* prev = nullptr;            // the pool as the previous pass of the same kind (forward / backward) left it: scales of the fp16 copies
    int next = 0, limit = 0;
    std::map<const void*, const float*> slots;  // tensor / panel pointer -> its slot array
    // second forward chain (frames [n1, B)): its own slot arrays, CHAIN2_OFF arrays above the first chain's and taken in the same
    // order, so that each chain's scales depend on its own frames only (deterministic) and one elementwise max after the join
    // gives the backward pass the ranges of the whole tensors
    std::map<const void*, const float*> slots2;
    int next2 = 0;
    bool chain2 = false;
    bool on = false;
    // the next slot array of the running pass (of the running chain); the ORDER of these calls pairs a tensor with its slots of one step ago
    float* take() {
        if (!on || !pool) return nullptr;
        if (chain2) {
            if (next2 >= RANGE_FWD) return nullptr;
            return pool + (size_t)(RANGE_FWD + next2++) * dgp::ABSMAX_SLOTS;
        }
        if (next >= limit) return nullptr;
        return pool + (size_t)(next++) * dgp::ABSMAX_SLOTS;
    }
    const float* of(const void* p) const {
        if (!on) return nullptr;
        if (chain2) {                     // the chain's own tensors first; weight panels are shared
            auto it2 = slots2.find(p);
            if (it2 != slots2.end()) return it2->second;
        }
        auto it = slots.find(p);
        return it == slots.end() ? nullptr : it->second;
    }
    void set(const void* p, const float* slot) {
        auto& m = chain2 ? slots2 : slots;
        if (slot) m[p] = slot; else m.erase(p);
    }
    // previous-step slots of the tensor that takes `slot` in this pass (the passes take their slots in the same order every step)
    const float* prev_of(const float* slot) const {
        if (!slot || !pool || !prev) return nullptr;
        long long idx = (slot - pool) / dgp::ABSMAX_SLOTS;
        if (idx < 0 || idx >= RANGE_POOL) return nullptr;
        if (idx >= RANGE_FWD && idx < 2 * RANGE_FWD) idx -= RANGE_FWD;      // chain 2 writes its frames of the same copy with the same scale
        return prev + idx * dgp::ABSMAX_SLOTS;
    }
};

// Per-trainer launch state that outlives a pass (two trainers, or a trainer created after another was destroyed, must not see each
// other's range maps, fp16 cell tables or copies).  A pass reaches it through its TrainPass; nothing here is bound to a thread.
struct TrainCtx {
    RangeCtx rng;
    std::unordered_map<const float*, const float*> cells;      // weight panel -> the same panel pre-split into fp16 cells
    std::unordered_map<const float*, const void*> cells1;      // ... -> its high-only H1 cells (16-bit tier, launch_pack_h1)
    // Weight gradients on a second stream (EXPERIMENTS.md section 6a (8)): the data-gradient chain is the critical path of the backward pass
    // and its 11-frame grids leave CUs idle; a layer's weight gradient only needs (x, dY) and is not needed before the finalisation
    // launches, so it runs on `s2` behind an event and the chain goes on (WgradSide).  The forward pass runs its second chain of frames there.
    hipStream_t s2 = nullptr;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    // fp16 high / low copies of retained activations and gradient buffers (ConvArgs::shadow), operands of wgrad_dma:
    // tensor base -> copy base (from the plan, per pass); tensor base -> previous-step range slots of the launch that WROTE the copy
    // in this pass (absent: no copy of the current contents exists)
    std::unordered_map<const void*, float*> shadow_base;
    std::unordered_map<const void*, const float*> shadow_prev;
    std::vector<int> h2_slots;                   // range slots of the tensors written as H2 with predicted scales in this pass
    ~TrainCtx() {
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        if (s2) (void)hipStreamDestroy(s2);
    }
    hipEvent_t take_event() {
        if (ev_next == ev_pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            ev_pool.push_back(e);
        }
        return ev_pool[ev_next++];
    }
    // `t` exists only as fp16 cells (an H2 / H1 tensor) scaled by the previous-step slots `pv`: weight gradients read it in place, and the
    // pass checks this step's range against the prediction at its end
    void note_cells(const void* t, const float* pv) {
        shadow_base[t] = const_cast<float*>(static_cast<const float*>(t));
        shadow_prev[t] = pv;
        const int idx = (int)((pv - rng.prev) / dgp::ABSMAX_SLOTS);
        if (std::find(h2_slots.begin(), h2_slots.end(), idx) == h2_slots.end()) h2_slots.push_back(idx);
    }
};

struct dgp_trainer {
    TrainCtx ctx;
    dgp_net* net = nullptr;
    std::vector<TLayer> tl;
    std::vector<std::string> names;
    std::vector<long long> offs, sizes;
    std::vector<int> is_stat;
    long long n_train = 0, n_stat = 0;
    float *params = nullptr, *grads = nullptr, *mom = nullptr, *stats = nullptr;
    double* d_sumsq = nullptr;        // TWO accumulators used in turn: the optimiser's kernel zeroes the other one for the next step (no fill launch)
    int sumsq_k = 0;
    float* d_gnorm = nullptr;
    // Adam's slots (dgp_adam_clip): allocated by the first Adam step or the first upload into them, so a momentum-only trainer holds none.
    // d_adam_pow: {beta1_power, beta2_power} twice, used in turn like d_sumsq -- pair adam_pow_k is current, the kernel writes the other
    float *adam_m = nullptr, *adam_v = nullptr, *d_adam_pow = nullptr;
    int adam_pow_k = 0;
    float* h_status = nullptr;        // pinned, device-visible: dgp_trainer_step_status' kernel writes [8 losses | gnorm | flag] straight into it
    float* d_rng_pool = nullptr;      // activation / gradient range slots (RANGE_POOL arrays), zeroed per pass
    float* d_rng_prev = nullptr;      // ... as the previous step left them (copied before the zeroing)
    int* d_fast_flag = nullptr;       // != 0: an H2 tensor of the last fast pass left its predicted range (the step must be repeated)
    bool fast_next = false;           // dgp_trainer_fast_mode: the next forward pass keeps blocks 2-4 as H2 tensors with predicted scales
    bool fwd_fast = false;            // what the last forward pass did (the backward pass reads its tensors accordingly)
    // precision tier (dgp_trainer_set_tier): 0 = parity (fp32-class arithmetic, fp32 retained activations); 1 = 16-bit: once a pass of
    // the same shapes has left its ranges behind, blocks 2-4 keep their retained activations AND their gradient tensors as H1 cells
    // (2 bytes per channel, scales predicted from the previous step's ranges, no fp32 twins), forward / data-gradient convs run one MFMA
    // per product on H1 operands and the weight gradients read both operands in place by LDS-DMA (wgrad_dma_h1).  fp32 master
    // weights, momentum, gradient accumulation (float atomics into fp32 dW), loss, block1 / stem / heads.  A step whose tensors left
    // their predicted ranges raises d_fast_flag and the host repeats it on the parity path.
    int tier = 0;
    int fwd_fmt = 0;                  // cell format of the last fast forward pass: 1 H2 (tuning builds' fast pass), 2 H1 (tier 1)
    void* d_h1_table = nullptr;       // PackH3Desc of every panel whose H1 cells are rebuilt per sync (tier 1)
    float* d_stem_rows = nullptr;     // tier 1: the stem's row panel [7 x 8 pixels][64][4] and its cells for stem_pool_fused_kernel, rebuilt per sync
    void* d_stem_cells = nullptr;
    bool fwd_stem_fused = false;      // the last forward pass ran the fused root block (no conv1 map, no fp32 pool output)
    // tier 1: both heads' data-gradient panels merged (pack_heads_dgrad_kernel), its range slots and its H1 cells; CT input channels
    float* d_hmT = nullptr;
    float* d_hm_rng = nullptr;
    void* d_hmT_h1 = nullptr;
    int hm_ct = 0, hm_nk = 0;
    bool fwd_feat32 = true;           // the last fast forward pass left an fp32 copy of the features (not when the heads' backward reads H1)
    // tier 1: what only a parity pass reads -- the H2 cells of every panel, the heads' 2x2-conv and data-gradient panels -- is not rebuilt by
    // every dgp_trainer_sync_weights but when a plain pass is about to run (refresh_parity_panels)
    bool parity_stale = false;
    int n_h1 = 0;
    float* d_wrng = nullptr;          // weight-panel range slots: [2 * n_layers] (forward panels, data-gradient panels), per sync
    void* d_pack_table = nullptr;     // PackDesc of every non-head layer (pack_all_kernel), built at the first sync
    int n_pack = 0;
    void* d_h3_table = nullptr;       // PackH3Desc of every panel whose cells are rebuilt per sync (DGP_TRAIN_CELLS)
    int n_h3 = 0;
    void* d_fin_table = nullptr;      // FinDesc of every non-head layer (deferred weight-gradient finalisation), per batch size
    int n_fin = 0, fin_B = -1, fin_h = -1, fin_w = -1;
    // Gradient groups (data-parallel training: the all-reduce of a group starts while the backward pass is still running).  The flat
    // gradient buffer is laid out in layer order and the pass finishes the layers back to front, so a group is a run of bottleneck
    // units: group 0 = the heads + the last units, ..., the LAST group = whatever is left + the stem.  Per group: the unit after whose
    // backward it is complete (-1: the end of the pass), its rows of the finalisation table, its float range in the flat buffer and
    // the event recorded behind its finalisation.
    struct GradGroup { int cut_ui = -1, fin_first = 0, fin_count = 0; long long lo = 0, hi = 0; hipEvent_t ev = nullptr; };
    std::vector<GradGroup> groups;
    std::vector<int> fin_of_layer;
    ~dgp_trainer() {
        for (void* q : {(void*)d_rng_pool, (void*)d_rng_prev, (void*)d_fast_flag, (void*)d_wrng, d_pack_table, d_fin_table, d_h3_table, d_h1_table, (void*)d_stem_rows, d_stem_cells, (void*)d_hmT, (void*)d_hm_rng, d_hmT_h1}) if (q) (void)hipFree(q);
        for (auto& g : groups) if (g.ev) (void)hipEventDestroy(g.ev);
        for (auto& t : tl) { if (t.d_wT) (void)hipFree(t.d_wT); if (t.d_wTh3) (void)hipFree(t.d_wTh3); if (t.d_wTh1) (void)hipFree(t.d_wTh1); }
        for (void* p : {(void*)params, (void*)grads, (void*)mom, (void*)stats, (void*)d_sumsq, (void*)d_gnorm, (void*)adam_m, (void*)adam_v, (void*)d_adam_pow})
            if (p) (void)hipFree(p);
        if (h_status) (void)hipHostFree(h_status);
    }
};

// The two switches that several trainer files read, each read once per process.
// A/B switch (DGP_WGRAD_DMA=0: no copies, wgrad_h3p as before)
inline const bool g_wgrad_dma = (dgp::dgp_tune("DGP_WGRAD_DMA", 1) != 0);

// weight panel -> the same panel pre-split into fp16 cells (filled by dgp_trainer_sync_weights): with the cells and both ranges the
// conv runs on the compute-side-split / LDS-DMA kernels of the inference engine
// Default on (DGP_TRAIN_CELLS=0: the trainer's convs split their weights in the loaders): the cells of all panels are rebuilt by ONE
// launch per sync (pack_h3_all_kernel), after which forward and data-gradient convs run the engine's compute-side-split / LDS-DMA /
// 16x16x32 kernels: 17.0 -> 16.2 ms per step.  (With one pack launch per layer and panel the packing cost what the kernels saved.)
inline const bool g_train_cells = (dgp::dgp_tune("DGP_TRAIN_CELLS", 1) != 0);

// One conv launch of the training step: a panel, the geometry as the kernels see it (a data gradient: the transposed conv), range keys, cell
// formats, the fp16 copy.  conv_call() / dgrad_call() give the common cases, a call site names what differs (as ConvCall in dgp_net.hip).
// conv_args() turns it into the kernels' ConvArgs; the pass (conv_launch) or a layer-level entry point adds ranges, cells and scales.
struct ConvCall {
    dgp_conv_desc d{};                          // N, grids, channels, taps, padding, ReLU, residual mode and extent
    const float* wpk = nullptr;                 // the panel as packed: nk K-steps x coutP columns
    int nk = 0, coutP = 0;
    const float *scale = nullptr, *bias = nullptr;
    const float *in = nullptr, *res = nullptr, *mask = nullptr;
    float* out = nullptr;
    int up = 0;                                 // > 1: the input is read on the zero-stuffed grid (data gradient of a strided conv)
    int out_mode = 0, dc_nj = 0;                // 1: a head's phase scatter with dc_nj channels per phase
    // in_key / out_key: the tensors under whose names this launch looks up / registers range slots when `in` / `out` are frame ranges
    // inside them (the forward pass as two chains of frames; each chain keeps its own slots, merged after the join)
    const void *in_key = nullptr, *out_key = nullptr;
    // fast pass: cell formats of the launch's tensors (0: fp32).  An H2 / H1 tensor's scale is the one predicted from the previous step's
    // slots of the tensor named by in_key / out_key / res_key.
    int in_fmt = 0, out_fmt = 0, res_fmt = 0, mask_fmt = 0;
    const void* res_key = nullptr;
    bool copy = true;                           // the output gets an fp16 copy where it has a region for one (backward: only gradients that a 128 x 128 weight-gradient tile will read)
    ConvCall& grid(int ho, int wo, int pt = 0, int pl = 0) { d.Ho = ho; d.Wo = wo; d.pad_t = pt; d.pad_l = pl; return *this; }
    ConvCall& strided(int s) { d.stride = s; return *this; }
    // residual [N, rH, rW, Cout]; mode s >= 1: read at (ho s, wo s), -2: the subsample shortcut's gradient on the 2x coarser grid
    ConvCall& residual(const float* r, int s, int rH, int rW) { res = r; d.res_stride = r ? s : 0; d.res_H = rH; d.res_W = rW; return *this; }
    ConvCall& gate(const float* m, int fmt = 0) { mask = m; mask_fmt = fmt; return *this; }      // out = 0 where m <= 0 (m as fp32 or as cells)
    ConvCall& linear() { d.relu = 0; return *this; }
    ConvCall& head_scatter(int nj) { out_mode = 1; dc_nj = nj; return *this; }
    ConvCall& keys(const void* ik, const void* ok) { in_key = ik; out_key = ok; return *this; }
    ConvCall& cells(int fmt, const void* rkey = nullptr) { in_fmt = out_fmt = fmt; res_fmt = rkey ? fmt : 0; res_key = rkey; return *this; }
    ConvCall& no_copy(bool none = true) { copy = !none; return *this; }
};
// Data gradient of the forward conv `fwd` (x [N, H, W, Cin] -> y [N, Ho, Wo, Cout]) as the launch the kernels see: the transposed conv
// dy -> dx [N, H, W, Cin] through the data-gradient panel wT (nkT K-steps x cinP columns), padding flipped, no affine, linear.  A strided
// conv reads dy on the zero-stuffed grid: the kernels' gather (`up`), or stuffed = true when dy IS the zero-stuffed tensor
// [N, stride Ho, stride Wo, Cout] (h1_zero_stuff).  The heads: fwd = their 2x2-conv form (head_wgrad_call's desc).
ConvCall dgrad_call(const dgp_conv_desc& fwd, const float* wT, int nkT, int cinP, const float* dy, float* dx, bool stuffed = false);
// What a launch is without a pass: tensors, panel, geometry and extents (fill_conv_geometry), up, out_mode, cell formats, gate.
int conv_args(dgp::ConvArgs& a, const ConvCall& c, const char* too_big);

// One operand of a weight gradient: the fp32 tensor, this step's range slots (null: unknown) and, where the operand also exists as fp16
// cells -- a copy its producer wrote, or the tensor itself in a fast pass -- the cells and the previous-step slots that scaled them
struct WgradOperand {
    const float* p = nullptr;
    const float* rng = nullptr;
    const void* cells = nullptr;
    const float* prev = nullptr;
};
// dWraw[(tap, ci)][co] = sum over pixels of x[m + tap][ci] * dy[m][co], colsum[co] = sum of dy[m][co]
struct WgradCall {
    dgp_conv_desc d{};                          // the forward conv: x [N, H, W, Cin] -> dy [N, Ho, Wo, Cout]
    WgradOperand x, dy;
    float *dwraw = nullptr, *colsum = nullptr;  // output scratch
    bool zeroed = false;                        // the scratch was zeroed for the whole pass
    // x exists only as cells (fast pass): the LDS-DMA tile is the only kernel that can read it, and copies that left their predicted range
    // raise the flag instead of falling back
    int* fail_flag = nullptr;
    bool h1 = false;                            // 16-bit tier: both operands are H1 tensors (in place or the H1 copy of a boundary tensor)
};
// a head's weight gradient: the 2x2-conv form (pad 1) on the feature grid, x [N, h, w, cin] and dy [N, h, w, cdy phase columns]
WgradCall head_wgrad_call(int N, int h, int w, int cin, int cdy, float* dwraw, float* colsum);

// The fused stem weight gradient (16-bit tier): the centred frames x [B, H, W, 4], d pool as an H1 tensor g [B, HP, WP, 64] with the slots
// g_prev that predict its scale, the pool's first-maximum record idx; slab: one row of 196 * 64 + 64 floats per workgroup (at most
// B * ceil(H1 / 4) * ceil(W1 / 32) of them); dw [49 * 4][64] and colsum [64] are accumulated
struct StemWgradCall {
    const float* x = nullptr; const void* g = nullptr; const unsigned char* idx = nullptr; const float* g_prev = nullptr;
    float *slab = nullptr, *dw = nullptr, *colsum = nullptr;
    int B = 0, H = 0, W = 0, H1 = 0, W1 = 0, HP = 0, WP = 0;
};

// ---- dgp_wgrad.hip ----
hipError_t wgrad_launch(const WgradCall& c, hipStream_t s);
void stem_wgrad_launch(const StemWgradCall& c, hipStream_t s);

// ---- dgp_train_pack.hip ----
int refresh_parity_panels(dgp_trainer* tr, hipStream_t s);
int trainer_owner_sync(void* owner, void* stream);            // dgp_net::owner_sync
hipError_t build_stem_cells(const float* panel, int CoutP, const float* mean_pixel, const float* panel_rng, float* rows, void* cells, hipStream_t s);
// pack_all_kernel over a device table of n_layers PackDesc; n_jobs 3: forward panels, data-gradient panels, folded BN; 1: forward panels only
void launch_pack_all(const void* table_dev, int n_layers, int n_jobs, const float* params, const float* stats, float eps, hipStream_t s);
// both heads' data-gradient panels side by side (pack_heads_dgrad_kernel): CT input channels, nkT K-steps x cinP columns
void launch_pack_heads_dgrad(const float* w0, int njt0, int cpad0, const float* w1, int njt1, int cpad1, int cin, int CT, int cinP, int nkT,
                             float* packed, float* rng, hipStream_t s);
// The scratch of a layer-level data gradient, [panel | its cells | 4 range slots | ones], and the panel packed into it from HWIO weights
// (pack_dgrad_kernel).  Slot 1 takes the panel's range; the other slots are the caller's.  bytes: the size the carve ends at.
struct DgradPanel {
    int nkT, cinP;
    float* panel; void* cells; float* rng; float* ones;
    size_t bytes;
    explicit DgradPanel(const dgp_conv_desc& d, void* scratch = nullptr);
    // zeroes the slots, packs w_hwio * scale (scale == NULL: ones, uploaded behind a stream synchronisation)
    int pack(const dgp_conv_desc& d, const float* w_hwio, const float* scale, hipStream_t s) const;
};

// ---- dgp_train.hip: the pass's element-wise kernels that the layer-level entry points launch too ----
void launch_f32_to_h1_pred(const float* x, long long n, const float* prev, void* out_h1, hipStream_t s);      // n floats, a multiple of 8
void launch_h1_to_f32_pred(const void* x_h1, long long n8, const float* prev, float* out, const void* gate_h1, hipStream_t s);
void launch_f32_to_shadow(const float* x, long long n8, const float* prev, void* out_h2, hipStream_t s);
// H1 dy [N, Ho, Wo, C] -> out [N, 2 Ho, 2 Wo, C], dy at the even positions and zeros elsewhere (N * 2 Ho * 2 Wo * C * 2 bytes)
hipError_t h1_zero_stuff(hipStream_t s, const void* dy_h1, int N, int Ho, int Wo, int C, void* out);
// every listed slot of `pool` against the scale its slot of `prev` predicts: *flag |= 1 | (slot + 1) << 8 where it left the range
int launch_h2_pred_check(const int* slots, int n, const float* pool, const float* prev, int* flag, const char* too_many, hipStream_t s);
void launch_head_gather_h1(const float* dsc0, const float* dsc1, int N, int h, int w, int njt0, int cpad0, int njt1, int cpad1, int CT,
                           const float* prev, void* out_h1, float* slot, hipStream_t s);
hipError_t heads_h1_param_grads(const WgradCall& wc, int njt0, int njt1, int cpad0, float* dw0, float* db0, float* dw1, float* db1, hipStream_t hs);
void launch_maxpool_fwd_idx(const float* c1, int nB, int h1, int w1, int hp, int wp, float* pool, uchar4* idx, uint2* y_h1, const float* y_prev,
                            hipStream_t s);
void launch_maxpool_bwd_idx(const float* c1, const float* dpool, const uchar4* idx, int B, int h1, int w1, int hp, int wp, float* dc1, hipStream_t s);
