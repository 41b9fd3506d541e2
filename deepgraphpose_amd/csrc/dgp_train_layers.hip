// Single layers of the training step as entry points (layer-level parity tests at the real shapes, sweep scripts): each one prepares its
// operands in a scratch buffer and then goes through the builders and launchers the pass itself uses (dgp_train.h).  No kernel of its own.
#include "dgp_train.h"

using namespace dgp;

extern "C" {

/* dWraw[(tap, ci)][co] = sum_m x[m + tap][ci] * dy[m][co] (HWIO order, Cin rows per tap), colsum[co] = sum_m dy[m][co].
 * With both ranges (DGP_ABSMAX_SLOTS floats each) the fp16-split kernel wgrad_h3p runs where the tile is 128 x 128, else wgrad_f32. */
int dgp_conv2d_wgrad(const dgp_conv_desc* d, const float* x, const float* dy, const float* x_absmax, const float* dy_absmax,
                     float* dw_raw, float* colsum, void* stream) {
    if (!d || !x || !dy || !dw_raw) return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad: null argument");
    if (d->Cin < 4 || (d->Cin & 3) || ((d->Cin / 4) & (d->Cin / 4 - 1)) || (d->Cout & 3))
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad: Cin must be 4 * 2^k, Cout a multiple of 4");
    if (!fits_descriptor({(double)d->N * d->H * d->W * d->Cin * 4, (double)d->N * d->Ho * d->Wo * d->Cout * 4}))
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad: tensor exceeds 4 GiB");
    // (layer-level call: no pass, the caller's ranges only)
    WgradCall c;
    c.d = *d; c.x = {x, x_absmax}; c.dy = {dy, dy_absmax}; c.dwraw = dw_raw; c.colsum = colsum;
    hipError_t e = wgrad_launch(c, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_conv2d_wgrad: ") + hipGetErrorString(e));
    return DGP_OK;
}

/* dgp_conv2d_wgrad through the LDS-DMA tile (wgrad_dma): x and dy are first copied into fp16 high / low cells with the scales that
 * x_prev / dy_prev (range slots "of the previous step") predict, as the producers' epilogues do inside the training step; the kernel
 * checks x_absmax / dy_absmax (this step's ranges) against them and runs the fp32-MFMA tile on x / dy where the copies are unusable.
 * scratch: 4 * (numel(x) + numel(dy)) device bytes. */
int dgp_conv2d_wgrad_shadow(const dgp_conv_desc* d, const float* x, const float* dy, const float* x_absmax, const float* dy_absmax,
                            const float* x_prev, const float* dy_prev, void* scratch, float* dw_raw, float* colsum, void* stream) {
    if (!d || !x || !dy || !dw_raw || !scratch || !x_absmax || !dy_absmax || !x_prev || !dy_prev)
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad_shadow: null argument");
    if (d->Cin < 16 || (d->Cin & 15) || ((d->Cin / 4) & (d->Cin / 4 - 1)) || (d->Cout & 7) || d->Cout < 128 || d->KH * d->KW * d->Cin < 128)
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad_shadow: Cin must be 16 * 2^k, Cout a multiple of 8, and the tile 128 x 128 (K, Cout >= 128)");
    if ((double)d->N * d->H * d->W * d->Cin * 4 > 4200000000.0 || (double)d->N * d->Ho * d->Wo * d->Cout * 4 > 4200000000.0)
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad_shadow: tensor exceeds 4 GiB");
    hipStream_t s = (hipStream_t)stream;
    const long long nx = (long long)d->N * d->H * d->W * d->Cin, ny = (long long)d->N * d->Ho * d->Wo * d->Cout;
    float* xs = (float*)scratch;
    float* dys = xs + nx;
    launch_f32_to_shadow(x, nx / 8, x_prev, xs, s);
    launch_f32_to_shadow(dy, ny / 8, dy_prev, dys, s);
    WgradCall c;
    c.d = *d; c.x = {x, x_absmax, xs, x_prev}; c.dy = {dy, dy_absmax, dys, dy_prev}; c.dwraw = dw_raw; c.colsum = colsum;
    hipError_t e = wgrad_launch(c, s);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_conv2d_wgrad_shadow: ") + hipGetErrorString(e));
    return DGP_OK;
}

/* dx = gate( convT(dy; w * scale) + dx_add ): the data gradient of the forward conv `d` (x [N,H,W,Cin] -> y [N,Ho,Wo,Cout]).
 * w_hwio: device HWIO weights; scale: [Cout] device or NULL; mask: [N,H,W,Cin] (gate: mask > 0) or NULL; dx_add: gradient of the
 * shortcut branch or NULL, on dx's grid (add_mode 1) or on the 2x coarser grid (add_mode -2: the subsample shortcut).
 * scratch: >= dgp_conv2d_dgrad_scratch_bytes(d) device bytes (data-gradient panel, its fp16 cells, range slots).
 * ranged bit 0: measure max |dy| and run the fp16-split kernels (what the trainer does), else the bf16x6 split; bit 1: `mask` is an H2
 * tensor (dgp_f32_to_h2 of the activation, any scale) as in the fast pass of the training step -- fp16-split kernels only. */
size_t dgp_conv2d_dgrad_scratch_bytes(const dgp_conv_desc* d) {
    return d ? DgradPanel(*d).bytes : 0;
}

int dgp_conv2d_dgrad(const dgp_conv_desc* d, const float* dy, const float* w_hwio, const float* scale, const float* mask,
                     const float* dx_add, int32_t add_mode, float* dx, void* scratch, int32_t ranged, void* stream) {
    if (!d || !dy || !w_hwio || !dx || !scratch) return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad: null argument");
    // (Cin < 64: dx goes through the 32-column fp32 tile, which reads the gate as fp32 -- garbage with H2 cells; found by scripts/fuzz_backward_layers.py)
    if ((ranged & 2) && (!(ranged & 1) || !mask || (d->Cin & 7) || d->Cin < 64))
        return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad: an H2 gate needs ranged bit 0, a mask and Cin % 8 == 0, Cin >= 64");
    if ((d->Cout & 31) || (d->Cin & 3)) return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad: Cout % 32, Cin % 4");
    hipStream_t s = (hipStream_t)stream;
    const DgradPanel pk(*d, scratch);
    float* const rng = pk.rng;                  // [0]: dy, [1]: panel, [2]: dx
    if (int rc = pk.pack(*d, w_hwio, scale, s)) return rc;
    const bool coarse = add_mode == -2;
    // (mask_fmt 1: the gate tensor is H2 -- fast pass of the training step: gate = stored value > 0)
    const ConvCall c = dgrad_call(*d, pk.panel, pk.nkT, pk.cinP, dy, dx)
                           .residual(dx_add, add_mode, coarse ? (d->H + 1) / 2 : d->H, coarse ? (d->W + 1) / 2 : d->W)
                           .gate(mask, (ranged & 2) ? 1 : 0);
    ConvArgs a{};
    if (int rc = conv_args(a, c, "dgp_conv2d_dgrad: tensor exceeds 4 GiB")) return rc;
    if (ranged & 1) {
        HIP_TRY(launch_absmax(dy, (long long)d->N * d->Ho * d->Wo * d->Cout, rng, s));
        HIP_TRY(launch_pack_h3(pk.panel, pk.nkT, pk.cinP, rng + ABSMAX_SLOTS, pk.cells, s));
        a.in_absmax = rng; a.w_absmax = rng + ABSMAX_SLOTS; a.wh3 = pk.cells; a.wh3_bytes = a.w_bytes;
        a.out_absmax = rng + 2 * ABSMAX_SLOTS;
    }
    HIP_TRY(launch_conv(a, pick_tile(a.M, a.CoutP, a.nk * BK, a.in_absmax && a.w_absmax), s));
    return DGP_OK;
}

/* ---- the same for the 16-bit tier: fp32 tensors in, converted to H1 tensors by the trainer's own converter (f32_to_h1_pred_kernel) with
 * the scales that "previous step" range slots predict, then the launchers of the 16-bit pass.  The H1 tensors stay in `scratch`. ---- */

/* H1 cells with the scale `prev` predicts -> fp32 (h1_to_f32_pred_kernel); gate_h1: an H1 tensor of the same shape or NULL */
int dgp_h1_to_f32_pred(const void* x_h1, size_t n_halves, const float* prev, const void* gate_h1, float* out, void* stream) {
    if (!x_h1 || !prev || !out || (n_halves & 7)) return fail(DGP_ERR_INVALID, "dgp_h1_to_f32_pred: null argument or a count that is no multiple of 8");
    const long long n8 = (long long)(n_halves / 8);
    launch_h1_to_f32_pred(x_h1, n8, prev, out, gate_h1, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

/* dgp_conv2d_wgrad on wgrad_dma_h1: scratch = [x as H1 | dy as H1] (2 * (numel(x) + numel(dy)) bytes).  *flag (device) is zeroed, then
 * takes the kernel's failure bits: 2 when a tensor left the range its predicted scale covers -- dw_raw and colsum are then zero, there is
 * no fp32 path behind this kernel. */
int dgp_conv2d_wgrad_h1(const dgp_conv_desc* d, const float* x, const float* dy, const float* x_absmax, const float* dy_absmax,
                        const float* x_prev, const float* dy_prev, void* scratch, float* dw_raw, float* colsum, int32_t* flag, void* stream) {
    if (!d || !x || !dy || !dw_raw || !scratch || !x_absmax || !dy_absmax || !x_prev || !dy_prev || !flag)
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad_h1: null argument");
    if (d->Cin < 16 || (d->Cin & 15) || ((d->Cin / 8) & (d->Cin / 8 - 1)) || (d->Cout & 7))
        return fail(DGP_ERR_INVALID, "dgp_conv2d_wgrad_h1: Cin must be 16 * 2^k, Cout a multiple of 8");
    hipStream_t s = (hipStream_t)stream;
    const long long nx = (long long)d->N * d->H * d->W * d->Cin, ny = (long long)d->N * d->Ho * d->Wo * d->Cout;
    char* xh = (char*)scratch;
    char* dyh = xh + 2 * nx;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    launch_f32_to_h1_pred(x, nx, x_prev, xh, s);
    launch_f32_to_h1_pred(dy, ny, dy_prev, dyh, s);
    WgradCall c;
    c.d = *d; c.x = {reinterpret_cast<const float*>(xh), x_absmax, xh, x_prev}; c.dy = {reinterpret_cast<const float*>(dyh), dy_absmax, dyh, dy_prev};
    c.dwraw = dw_raw; c.colsum = colsum; c.fail_flag = flag; c.h1 = true;
    hipError_t e = wgrad_launch(c, s);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_conv2d_wgrad_h1: ") + hipGetErrorString(e));
    return DGP_OK;
}

/* dgp_conv2d_dgrad as an H1 -> H1 launch.  scratch: dgp_conv2d_dgrad_scratch_bytes(d) bytes as in dgp_conv2d_dgrad (panel, its high-only
 * cells, range slots), then [dy as H1][dx_add as H1][stride 2: dy zero-stuffed, N x 2 Ho x 2 Wo x Cout halves].  gate_h1: the gate as H1
 * cells or NULL.  *flag (device, may be NULL): zeroed, then 1 | (1 << 8) when dx left the range dx_prev predicts (the pass's own check). */
int dgp_conv2d_dgrad_h1(const dgp_conv_desc* d, const float* dy, const float* w_hwio, const float* scale, const void* gate_h1,
                        const float* dx_add, int32_t add_mode, const float* dy_prev, const float* dx_prev, const float* add_prev,
                        void* scratch, void* dx_h1, int32_t* flag, void* stream) {
    if (!d || !dy || !w_hwio || !dx_h1 || !scratch || !dy_prev || !dx_prev || (dx_add && !add_prev))
        return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad_h1: null argument");
    if ((d->Cout & 63) || (d->Cin & 63)) return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad_h1: Cin % 64, Cout % 64 (a K-step is 64 channels)");
    if (d->stride != 1 && d->stride != 2) return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad_h1: stride 1 or 2");
    if (dx_add && add_mode != 1 && add_mode != -2) return fail(DGP_ERR_INVALID, "dgp_conv2d_dgrad_h1: add_mode 1 or -2");
    hipStream_t s = (hipStream_t)stream;
    const DgradPanel pk(*d, scratch);
    float* const rng = pk.rng;             // [0]: dy, [1]: panel, [2]: dx
    const long long ny = (long long)d->N * d->Ho * d->Wo * d->Cout;
    const int aH = add_mode == -2 ? (d->H + 1) / 2 : d->H, aW = add_mode == -2 ? (d->W + 1) / 2 : d->W;
    const long long na = dx_add ? (long long)d->N * aH * aW * d->Cin : 0;
    char* const dyh = (char*)scratch + pk.bytes;
    char* const addh = dyh + 2 * ny;
    char* const zs = addh + 2 * na;
    if (int rc = pk.pack(*d, w_hwio, scale, s)) return rc;
    if (flag) HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    HIP_TRY(launch_pack_h1(pk.panel, pk.nkT, pk.cinP, rng + ABSMAX_SLOTS, pk.cells, s));
    HIP_TRY(launch_absmax(dy, ny, rng, s));
    launch_f32_to_h1_pred(dy, ny, dy_prev, dyh, s);
    if (dx_add) launch_f32_to_h1_pred(dx_add, na, add_prev, addh, s);
    const bool stuffed = d->stride == 2;       // a stride-2 layer: dy on the zero-stuffed 2 Ho x 2 Wo grid
    if (stuffed) HIP_TRY(h1_zero_stuff(s, dyh, d->N, d->Ho, d->Wo, d->Cout, zs));
    const float* const res = dx_add ? reinterpret_cast<const float*>(addh) : nullptr;
    const ConvCall c = dgrad_call(*d, pk.panel, pk.nkT, pk.cinP, reinterpret_cast<const float*>(stuffed ? zs : dyh), reinterpret_cast<float*>(dx_h1), stuffed)
                           .residual(res, add_mode, aH, aW).cells(2, res).gate(reinterpret_cast<const float*>(gate_h1), gate_h1 ? 2 : 0);
    ConvArgs a{};
    if (int rc = conv_args(a, c, "dgp_conv2d_dgrad_h1: tensor exceeds 4 GiB")) return rc;
    a.in_scale_dev = dy_prev; a.out_scale_dev = dx_prev; a.res_scale_dev = dx_add ? add_prev : nullptr;
    a.in_absmax = rng; a.w_absmax = rng + ABSMAX_SLOTS; a.wh3 = pk.cells; a.wh3_bytes = a.w_bytes;
    a.out_absmax = rng + 2 * ABSMAX_SLOTS;
    hipError_t e = launch_conv(a, pick_tile(a.M, a.CoutP, a.nk * BK, true), s);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_conv2d_dgrad_h1: ") + hipGetErrorString(e));
    const int slot0 = 0;                   // dx's measured range against dx_prev, each as a pool of one slot array
    if (flag) (void)launch_h2_pred_check(&slot0, 1, rng + 2 * ABSMAX_SLOTS, dx_prev, reinterpret_cast<int*>(flag), "", s);
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

/* stem_wgrad_h1_kernel + stem_wgrad_reduce_kernel as backward_root launches them.  scratch: [d pool as H1: 2 * numel(dpool) bytes][slab:
 * B * ceil(H1 / 4) * ceil(W1 / 32) rows of (196 * 64 + 64) floats].  dw [49 * 4][64] and colsum [64] are overwritten. */
int dgp_stem_wgrad_h1(const float* x_centred, const float* dpool, const float* dpool_prev, const uint8_t* idx, int32_t B, int32_t H, int32_t W,
                      int32_t H1, int32_t W1, int32_t HP, int32_t WP, void* scratch, float* dw, float* colsum, void* stream) {
    if (!x_centred || !dpool || !dpool_prev || !idx || !scratch || !dw || !colsum) return fail(DGP_ERR_INVALID, "dgp_stem_wgrad_h1: null argument");
    if (B < 1 || H < 1 || W < 1 || H1 != (H + 1) / 2 || W1 != (W + 1) / 2 || HP != (H1 + 1) / 2 || WP != (W1 + 1) / 2)
        return fail(DGP_ERR_INVALID, "dgp_stem_wgrad_h1: the maps must be those of the root block (conv 7x7 / 2, pool 3x3 / 2, SAME)");
    hipStream_t s = (hipStream_t)stream;
    const long long ng = (long long)B * HP * WP * 64;
    launch_f32_to_h1_pred(dpool, ng, dpool_prev, scratch, s);
    HIP_TRY(hipMemsetAsync(dw, 0, (size_t)196 * 64 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(colsum, 0, 64 * sizeof(float), s));
    StemWgradCall sa;
    sa.x = x_centred; sa.g = scratch; sa.idx = idx; sa.g_prev = dpool_prev;
    sa.dw = dw; sa.colsum = colsum;
    sa.B = B; sa.H = H; sa.W = W; sa.H1 = H1; sa.W1 = W1; sa.HP = HP; sa.WP = WP;
    sa.slab = reinterpret_cast<float*>((char*)scratch + (((size_t)ng * 2 + 255) & ~(size_t)255));
    stem_wgrad_launch(sa, s);
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

/* ---- the root block's pool and its fused form as layers (tests): the launches of forward_root / backward_root / the inference engine ---- */
static bool root_pool_maps(int B, int H1, int W1, int HP, int WP) {
    return B >= 1 && H1 >= 1 && W1 >= 1 && HP == (H1 + 1) / 2 && WP == (W1 + 1) / 2;
}

/* forward_root's unfused pool: c1 [B,H1,W1,64] fp32 -> pool [B,HP,WP,64] fp32, idx [B,HP,WP,64] bytes (position a * 3 + b of each window's
 * first maximum over its valid positions), and with prev + pool_h1 the H1 copy of the pool output at the scale prev predicts. */
int dgp_maxpool_fwd_idx(const float* c1, int32_t B, int32_t H1, int32_t W1, int32_t HP, int32_t WP, const float* prev, float* pool, uint8_t* idx,
                        void* pool_h1, void* stream) {
    if (!c1 || !pool || !idx || (!prev) != (!pool_h1)) return fail(DGP_ERR_INVALID, "dgp_maxpool_fwd_idx: null argument, or only one of prev / pool_h1");
    if (!root_pool_maps(B, H1, W1, HP, WP)) return fail(DGP_ERR_INVALID, "dgp_maxpool_fwd_idx: the maps must be those of the root block's pool (3x3 / 2, SAME)");
    launch_maxpool_fwd_idx(c1, B, H1, W1, HP, WP, pool, reinterpret_cast<uchar4*>(idx), reinterpret_cast<uint2*>(pool_h1), prev, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

/* backward_root's pool backward: dc1 [B,H1,W1,64] = (c1 > 0) * the gradient of every window whose record names the pixel; c1 == NULL: no gate */
int dgp_maxpool_bwd_idx(const float* c1, const float* dpool, const uint8_t* idx, int32_t B, int32_t H1, int32_t W1, int32_t HP, int32_t WP,
                        float* dc1, void* stream) {
    if (!dpool || !idx || !dc1) return fail(DGP_ERR_INVALID, "dgp_maxpool_bwd_idx: null argument");
    if (!root_pool_maps(B, H1, W1, HP, WP)) return fail(DGP_ERR_INVALID, "dgp_maxpool_bwd_idx: the maps must be those of the root block's pool (3x3 / 2, SAME)");
    launch_maxpool_bwd_idx(c1, dpool, reinterpret_cast<const uchar4*>(idx), B, H1, W1, HP, WP, dc1, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return DGP_OK;
}

/* stem_pool_fused_kernel on weights given as HWIO [7,7,3,64]: the forward panel (pack_all_kernel's job 0), the stem cells (build_stem_cells)
 * and launch_stem_pool_fused.  cells 1: H2 pool cells (the parity tier's inference), 2: H1 (the 16-bit tier).  The scale is 2^out_exp, or with
 * out_prev the one those range slots predict (the training step); idx: the first-maximum record [B,HP,WP,64], training step only.
 * scratch: [PackDesc | panel range slots | panel | row panel | cells]. */
size_t dgp_root_block_scratch_bytes(void) { return 256 + ABSMAX_SLOTS * sizeof(float) + (size_t)3 * 56 * 64 * 4 * sizeof(float); }

int dgp_root_block(const uint8_t* frames, int32_t B, int32_t H, int32_t W, const float* w_hwio, const float* bn_scale, const float* bn_bias,
                   const float* mean_pixel, int32_t cells, int32_t out_exp, const float* out_prev, uint8_t* idx, void* scratch, void* out,
                   float* out_absmax, void* stream) {
    if (B < 1 || H < 1 || W < 1 || (long long)B * H * W * 3 >= (1LL << 31))
        return fail(DGP_ERR_INVALID, "dgp_root_block: the frame batch must be smaller than 2^31 bytes");
    if (!frames || !w_hwio || !bn_scale || !bn_bias || !mean_pixel || !scratch || !out || !out_absmax)
        return fail(DGP_ERR_INVALID, "dgp_root_block: null argument");
    if (cells != 1 && cells != 2) return fail(DGP_ERR_INVALID, "dgp_root_block: cells 1 (H2) or 2 (H1)");
    if ((out_prev || idx) && cells != 2) return fail(DGP_ERR_INVALID, "dgp_root_block: a predicted scale and the record belong to the 16-bit tier (H1 cells)");
    if (idx && !out_prev) return fail(DGP_ERR_STATE, "16-bit tier: the root block's output has no predicted range");
    static_assert(sizeof(PackDesc) <= 256, "the table's slot in the scratch");
    hipStream_t s = (hipStream_t)stream;
    char* sp = (char*)scratch;
    PackDesc* table = reinterpret_cast<PackDesc*>(sp); sp += 256;
    float* wrng = (float*)sp; sp += ABSMAX_SLOTS * sizeof(float);
    const size_t nrow = (size_t)56 * 64 * 4;
    float* panel = (float*)sp; sp += nrow * sizeof(float);
    float* rows = (float*)sp; sp += nrow * sizeof(float);
    void* wcells = sp;
    PackDesc d{};                 // conv1 as the trainer's table describes it: 49 taps, 3 real input channels in slots of 4, 64 columns
    d.taps = 49; d.cin_real = 3; d.cin = 4; d.cout = 64; d.coutP = 64; d.nchunks_f = nk_for(7, 7, 4) * 8;
    d.d_w = panel; d.rng_f = wrng;
    HIP_TRY(hipMemsetAsync(wrng, 0, ABSMAX_SLOTS * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(out_absmax, 0, ABSMAX_SLOTS * sizeof(float), s));
    HIP_TRY(hipMemcpyAsync(table, &d, sizeof(d), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    launch_pack_all(table, 1, 1, w_hwio, nullptr, 0.f, s);
    HIP_TRY(build_stem_cells(panel, 64, mean_pixel, wrng, rows, wcells, s));
    hipError_t e = launch_stem_pool_fused(frames, B, H, W, wcells, wrng, bn_scale, bn_bias, mean_pixel[0], mean_pixel[1], mean_pixel[2],
                                          out_prev ? 0.f : ldexpf(1.f, out_exp), reinterpret_cast<float*>(out), out_absmax, s, cells == 2 ? 1 : 0,
                                          out_prev, idx);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_root_block: ") + hipGetErrorString(e));
    return DGP_OK;
}

/* backward_heads_h1's sequence on one stream: gather both heads' loss gradients into one H1 tensor of heads_ct(nj) columns, pack the merged
 * data-gradient panel, one weight-gradient launch, the two finalisations, one 2x2-tap H1 data gradient gated by the features.
 * scratch (bytes, each part rounded up to 256): [feat as H1: 2 N h w Cin][merged gradient as H1: 2 N h w CT][panel: nk 8 cinP 16][its cells:
 * half of that][dwraw: 4 Cin CT floats][colsum: 2 CT floats][4 range slots: features, merged gradient, panel, d features]. */
int dgp_heads_backward_h1(const float* feat, const float* feat_prev, const float* dscmap, const float* dlocref, const float* dph_prev,
                          const float* w_part, const float* w_locref, const float* dfeat_prev, int32_t N, int32_t h, int32_t w, int32_t Cin,
                          int32_t nj, void* scratch, float* dw_part, float* db_part, float* dw_locref, float* db_locref, void* dfeat_h1,
                          int32_t* flag, void* stream) {
    if (!feat || !feat_prev || !dscmap || !dlocref || !dph_prev || !w_part || !w_locref || !dfeat_prev || !scratch || !dw_part || !db_part ||
        !dw_locref || !db_locref || !dfeat_h1 || !flag)
        return fail(DGP_ERR_INVALID, "dgp_heads_backward_h1: null argument");
    if (N < 1 || h < 1 || w < 1 || nj < 1 || Cin < 64 || ((Cin / 8) & (Cin / 8 - 1)))
        return fail(DGP_ERR_INVALID, "dgp_heads_backward_h1: Cin must be 64 * 2^k");
    const int njt0 = nj, njt1 = 2 * nj, cpad0 = next_pow2(4 * njt0), cpad1 = next_pow2(4 * njt1);
    const int CT = heads_ct(nj), nkT = nk_for(2, 2, CT), cinP = coutp_for(Cin);
    // (the trainer's condition for the merged panel, dgp_trainer_sync_weights)
    if (!(cpad0 + cpad1 <= CT && (nkT % 2) == 0 && cinP % 64 == 0))
        return fail(DGP_ERR_INVALID, "dgp_heads_backward_h1: the merged panel does not take these head widths");
    hipStream_t s = (hipStream_t)stream;
    auto up256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const long long M = (long long)N * h * w;
    const size_t pbytes = (size_t)nkT * 8 * cinP * 16;
    char* sp = (char*)scratch;
    char* featH = sp; sp += up256((size_t)M * Cin * 2);
    char* DPH = sp; sp += up256((size_t)M * CT * 2);
    float* panel = (float*)sp; sp += up256(pbytes);
    void* cells = sp; sp += up256(pbytes / 2);
    float* dwraw = (float*)sp; sp += up256((size_t)4 * Cin * CT * sizeof(float));
    float* colsum = (float*)sp; sp += up256((size_t)2 * CT * sizeof(float));
    float* rng = (float*)sp;               // [0]: features, [1]: merged gradient, [2]: panel, [3]: d features
    HIP_TRY(hipMemsetAsync(rng, 0, 4 * ABSMAX_SLOTS * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    HIP_TRY(launch_absmax(feat, M * Cin, rng, s));
    launch_f32_to_h1_pred(feat, M * Cin, feat_prev, featH, s);
    float* slot_dph = rng + ABSMAX_SLOTS;
    launch_head_gather_h1(dscmap, dlocref, N, h, w, njt0, cpad0, njt1, cpad1, CT, dph_prev, DPH, slot_dph, s);
    launch_pack_heads_dgrad(w_part, njt0, cpad0, w_locref, njt1, cpad1, Cin, CT, cinP, nkT, panel, rng + 2 * ABSMAX_SLOTS, s);
    HIP_TRY(launch_pack_h1(panel, nkT, cinP, rng + 2 * ABSMAX_SLOTS, cells, s));
    WgradCall wc = head_wgrad_call(N, h, w, Cin, CT, dwraw, colsum);
    wc.x = {reinterpret_cast<const float*>(featH), rng, featH, feat_prev};
    wc.dy = {reinterpret_cast<const float*>(DPH), slot_dph, DPH, dph_prev};
    wc.fail_flag = reinterpret_cast<int*>(flag); wc.h1 = true;
    hipError_t e = heads_h1_param_grads(wc, njt0, njt1, cpad0, dw_part, db_part, dw_locref, db_locref, s);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_heads_backward_h1: weight gradient: ") + hipGetErrorString(e));
    // d features: the heads' 2x2-conv form over the merged tensor, as backward_heads_h1 builds it
    const ConvCall c = dgrad_call(wc.d, panel, nkT, cinP, reinterpret_cast<const float*>(DPH), reinterpret_cast<float*>(dfeat_h1))
                           .cells(2).gate(reinterpret_cast<const float*>(featH), 2);
    ConvArgs a{};
    if (int rc = conv_args(a, c, "dgp_heads_backward_h1: tensor exceeds 4 GiB")) return rc;
    a.in_scale_dev = dph_prev; a.out_scale_dev = dfeat_prev;
    a.in_absmax = slot_dph; a.w_absmax = rng + 2 * ABSMAX_SLOTS; a.wh3 = cells; a.wh3_bytes = a.w_bytes;
    a.out_absmax = rng + 3 * ABSMAX_SLOTS;
    e = launch_conv(a, pick_tile(a.M, a.CoutP, a.nk * BK, true), s);
    if (e != hipSuccess) return fail(DGP_ERR_HIP, std::string("dgp_heads_backward_h1: data gradient: ") + hipGetErrorString(e));
    return DGP_OK;
}

}  // extern "C"
