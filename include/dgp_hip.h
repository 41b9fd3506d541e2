/*
 * dgp_hip.h -- C-ABI of libdgp_hip.so, the MI355X (gfx950) engine for the Deep Graph
 * Pose hot path.  Plain pointers and sizes only; every device pointer is memory the
 * CALLER owns (e.g. torch tensors), `stream` is a hipStream_t passed as void*.
 *
 * The reference (paninski-lab/deepgraphpose) has no FFI: its boundary for this path is
 * one TF-1.x session call.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root; PET = src/DeepLabCut/deeplabcut/
 * pose_estimation_tensorflow, DGP = src/deepgraphpose):
 *
 *   dgp_forward        sess.run(scmap[,locref], {inputs: frames})   DGP/models/eval.py:328
 *                      graph: PET/nnet/pose_net.py:36-54 (extract_features) +
 *                             DGP/models/fitdgp_util.py:18-74 (dgp_prediction_layer)
 *   dgp_soft_argmax    argmax_2d_from_cm                            DGP/models/fitdgp_util.py:342-402
 *                      + likelihood read-out                        DGP/models/eval.py:331-343
 *   dgp_hard_argmax    argmax_pose_predict                          PET/nnet/predict.py:62-77
 *   dgp_infer          sess.run([mu_n, scmap]) + read-out           DGP/models/eval.py:306-345
 *   dgp_soft_argmax_locref   softmax-weighted locref offset         DGP/models/eval.py:757-786
 *   dgp_infer_packed_locref  the same loop with location refinement: DLC's own video analysis always applies the offsets
 *                      (PET/nnet/predict.py:62-77); the soft form is evaluate_dgp's loc_ref_calc='dgp' (DGP/models/eval.py:752-786)
 *   dgp_net_create /   setup_dgp_eval_graph (graph build + Saver.restore)
 *   dgp_net_load_weights                                            DGP/models/eval.py:147-214
 *
 * All functions return 0 on success or a negative dgp_status; dgp_last_error() gives a
 * thread-local message.  Launches are asynchronous on `stream`.  Functions that synchronise say so at their
 * declaration; the ones on the hot path are: the FIRST dgp_forward / dgp_infer after dgp_net_load_weights,
 * dgp_net_set_tier, dgp_net_recalibrate or a reported range overflow (the calibration pass reads every
 * layer's tracked range: one stream sync + 1 KB copy per layer, see "H2" below), dgp_net_range_status,
 * dgp_net_load_weights and the layer-level test entry points dgp_chain_h2 / dgp_unit_h2.  Every other
 * forward / infer call enqueues and returns.
 * A dgp_net handle is bound to the device current at creation and is not thread-safe.
 */
#ifndef DGP_HIP_H
#define DGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGP_ABI_VERSION 1

typedef enum dgp_status {
    DGP_OK = 0,
    DGP_ERR_INVALID = -1,     /* bad argument / shape */
    DGP_ERR_HIP = -2,         /* HIP runtime error (see dgp_last_error) */
    DGP_ERR_MISSING = -3,     /* a required weight tensor was not supplied */
    DGP_ERR_STATE = -4        /* e.g. forward before load_weights */
} dgp_status;

typedef struct dgp_net dgp_net;   /* opaque */

typedef struct dgp_net_desc {
    int32_t depth;        /* 50 | 101 | 152 (net_type resnet_50 / resnet_101, PET/nnet/pose_net.py:14-16) */
    int32_t num_joints;   /* cfg.num_joints */
    int32_t in_h, in_w;   /* frame size */
    int32_t max_batch;
    int32_t with_locref;  /* build pose/locref_pred head too (cfg.location_refinement) */
    float   mean_pixel[3];/* cfg.mean_pixel, RGB (PET/default_config.py:23) */
    float   bn_eps;       /* slim resnet_arg_scope epsilon, 1e-5 */
} dgp_net_desc;

/* One named weight tensor in the TF variable layout (HWIO convs, [kh,kw,Cout,Cin]
 * transposed convs, [C] vectors), fp32, host memory. */
typedef struct dgp_tensor_view {
    const char*  name;    /* TF variable name, e.g. "resnet_v1_50/conv1/weights" */
    const float* data;
    int32_t      ndim;
    int64_t      shape[4];
} dgp_tensor_view;

int          dgp_version(void);
/* 1 when the library was built with -DDGP_TUNING (tuning knobs read from the environment, the opt-in kernels that measured slower
 * compiled in), 0 for the product build.  No reference counterpart (build introspection for the tests). */
int          dgp_tuning_build(void);
/* Host-only helper: CRC-32C (Castagnoli) of a byte range, continuing from `crc` (0 to start).  Used for the
 * per-tensor checksums of TF tensor bundles that tf.train.Saver writes/verifies (DGP/models/fitdgp.py:149-171). */
uint32_t     dgp_crc32c(const void* data, size_t n, uint32_t crc);
const char*  dgp_last_error(void);

int  dgp_net_create(const dgp_net_desc* desc, dgp_net** out);
void dgp_net_destroy(dgp_net* net);
/* Copies + repacks (k-chunked weight panels, BN folded to scale/bias).  Synchronous. */
int  dgp_net_load_weights(dgp_net* net, const dgp_tensor_view* tensors, int32_t n);
int  dgp_net_workspace_bytes(const dgp_net* net, int32_t batch, size_t* out_bytes);
/* Output geometry of the heads: scoremap is [batch, out_h, out_w, num_joints]. */
int  dgp_net_output_dims(const dgp_net* net, int32_t* out_h, int32_t* out_w,
                         int32_t* feat_h, int32_t* feat_w);
/* Number of conv-stack kernel launches of one forward and their algorithmic FLOPs. */
int  dgp_net_stats(const dgp_net* net, int32_t batch, int32_t* n_launches, double* conv_flops);

/* frames: device uint8 [batch, in_h, in_w, 3] NHWC (RGB).
 * scmap : device fp32 [batch, out_h, out_w, nj]      (raw logits, pose/part_pred)
 * locref: device fp32 [batch, out_h, out_w, 2*nj] or NULL
 * features: optional device fp32 [batch, feat_h, feat_w, 2048] copy-out, or NULL */
int  dgp_forward(dgp_net* net, const uint8_t* frames, int32_t batch, void* workspace,
                 size_t workspace_bytes, float* scmap, float* locref, float* features,
                 void* stream);

/* DGP soft-argmax + likelihood window.
 * scmap [B,H,W,C] fp32 -> mu [B,C,2] (row, col) fp32, conf [B,C] fp32 (sigmoid of the raw
 * logit at the window arg-max), idx [B,C,2] int32 (row, col), pmap optional [B,H,W,C].
 * Any H x W (the reference's placeholders are [None, None, None, nj]): maps up to 38 400 cells are held in LDS, larger ones
 * stream from global memory with the same arithmetic.
 * gauss_len must be 1..7 (here, in dgp_infer and in dgp_infer_packed; DGP_ERR_INVALID otherwise): the blur has 2 gauss_len + 1
 * taps, and gauss_len 0 would make them 0/0.  A map whose mu is NaN (a +inf or NaN logit) reports idx (0, 0). */
int  dgp_soft_argmax(const float* scmap, int32_t B, int32_t H, int32_t W, int32_t C,
                     float gamma, int32_t gauss_len, float* mu, float* conf, int32_t* idx,
                     float* pmap, void* stream);

/* dgp_soft_argmax plus the location-refinement read-out in the same launch: locref [B,H,W,2C] fp32 (pose/locref_pred, channel 2c = dx,
 * 2c + 1 = dy of joint c: PET/nnet/predict.py:62-77, targets built by compute_target_part_scoremap), 8-byte aligned ->
 * offs [B,C,2] = sum(p * locref) / sum(p) over the normalised blurred softmax p that mu is the expectation under: the softmax-weighted
 * offset of DGP/models/eval.py:757-786, NOT yet scaled by locref_stdev.  mu, conf, idx and pmap are bit-identical to dgp_soft_argmax's
 * on the same scmap; the same argument checks apply (gauss_len 1..7).  A map with a +inf or NaN logit gives NaN offs. */
int  dgp_soft_argmax_locref(const float* scmap, const float* locref, int32_t B, int32_t H, int32_t W, int32_t C,
                            float gamma, int32_t gauss_len, float* mu, float* conf, int32_t* idx, float* offs,
                            float* pmap, void* stream);

/* argmax_2d_from_cm's `th` branch (DGP/models/fitdgp_util.py:377-388; unused by the reference's drivers): on the pmap that
 * dgp_soft_argmax wrote, per (frame, joint) map: values below th * max become 0, the map is renormalised IN PLACE and
 * mu [B,C,2] (row, col) is its expectation. */
int  dgp_pmap_threshold(float* pmap, int32_t B, int32_t H, int32_t W, int32_t C, float th, float* mu, void* stream);

/* DLC hard arg-max over sigmoid(scmap).  idx [B,C,2] (row, col), prob [B,C],
 * offs [B,C,2] = locref[b,row,col,2c..2c+1] (dx, dy; NOT yet scaled by locref_stdev) or
 * zeros when locref == NULL.
 * Order of np.argmax: the first row-major maximum; a NaN counts as the maximum and the FIRST NaN wins (an all-NaN map gives
 * idx (0, 0) and a NaN prob).  idx always lies inside the map, so the locref read does too. */
int  dgp_hard_argmax(const float* scmap, const float* locref, int32_t B, int32_t H, int32_t W,
                     int32_t C, int32_t* idx, float* prob, float* offs, void* stream);

/* Fused A1..A4: frames -> (mu, conf, idx); scoremap stays in the workspace unless
 * scmap_out != NULL. */
int  dgp_infer(dgp_net* net, const uint8_t* frames, int32_t batch, void* workspace,
               size_t workspace_bytes, float gamma, int32_t gauss_len, float* mu, float* conf,
               int32_t* idx, float* scmap_out, void* stream);

/* Same, written as ONE packed record per (frame, joint): traj [batch, nj, 5] fp32 lanes = (row, col, likelihood, iy, ix) with
 * the two window indices as int32 bit patterns in lanes 3..4.  This is the layout of the per-video trajectory that the
 * frame-sharded ranks exchange with a single RCCL all-gather; writing it here keeps torch's cat / copy
 * kernels out of the per-batch loop. */
int  dgp_infer_packed(dgp_net* net, const uint8_t* frames, int32_t batch, void* workspace,
                      size_t workspace_bytes, float gamma, int32_t gauss_len, float* traj,
                      float* scmap_out, void* stream);

/* dgp_infer_packed with location refinement: the forward also runs the locref head (into locref_out, or the workspace when NULL) and
 * ONE read-out launch writes traj [batch, nj, 7] fp32 lanes.
 *   mode 1 ("dgp"): (row, col, likelihood, iy, ix, dx, dy) = dgp_soft_argmax_locref's mu, conf, idx, offs
 *                   (DGP/models/eval.py:752-786: soft-argmax + softmax-weighted offset);
 *   mode 2 ("dlc"): (iy as float, ix as float, prob, iy, ix, dx, dy) = dgp_hard_argmax's idx, prob, offs
 *                   (PET/nnet/predict.py:62-77: arg-max of the sigmoid + the offset at that cell; gamma / gauss_len are only checked).
 * Lanes 0..4 of mode 1 are dgp_infer_packed's record, bit for bit; dx, dy are raw head outputs (multiply by locref_stdev).
 * A net created without with_locref: DGP_ERR_INVALID.  The heads own no activation scale: a net calibrated by dgp_infer_packed stays
 * calibrated for this entry and the other way round. */
int  dgp_infer_packed_locref(dgp_net* net, const uint8_t* frames, int32_t batch, void* workspace,
                             size_t workspace_bytes, float gamma, int32_t gauss_len, int32_t mode, float* traj,
                             float* scmap_out, float* locref_out, void* stream);

/* ---- measurement: hipEvent pairs around every launch of dgp_forward / dgp_infer, recorded on
 * the caller's stream (no syncs until dgp_net_profile_launch reads them).  Used by bench.py for
 * the roofline object; the reference's only timing is time.time() around sess.run
 * (DGP/models/fitdgp.py:817-828). */
/* Change the frame size of an existing net (weights stay).  DLC's step-0 loader feeds a differently scaled /
 * cropped image every iteration (pose_defaultdataset.py:131-196: placeholders [1, None, None, 3]); workspaces
 * are sized per call from the current geometry. */
int  dgp_net_set_input_size(dgp_net* net, int32_t in_h, int32_t in_w);

int  dgp_net_profile_begin(dgp_net* net, int32_t max_steps);
int  dgp_net_profile_end(dgp_net* net, int32_t* n_steps, int32_t* n_launches);
/* Average duration (ms, over the profiled steps), name and algorithmic FLOPs of launch i. */
int  dgp_net_profile_launch(dgp_net* net, int32_t launch, char* name, int32_t name_cap,
                            double* flops, double* avg_ms);

/* ---- DGP loss, forward + backward w.r.t. the head outputs (dgp_loss in DGP/models/fitdgp.py:848-1144).
 * Replaces the loss sub-graph evaluated inside sess.run([loss, train_op]) (fitdgp.py:818).
 * Marker id = frame_in_batch * nj + joint (DGP/dataset.py:187-239). */
typedef struct dgp_loss_desc {
    int32_t nt, H, W, nj, nl;             /* frames in batch, scoremap size, joints, limbs (rows of S0) */
    int32_t n_visible, n_hidden;          /* lengths of visible_marker / hidden_marker */
    int32_t gm2, gm3;                     /* hidden-loss variants: gm2 in {0,1,2}, gm3 in {0,3} (fitdgp.py:994-1034) */
    int32_t gauss_len, huber;             /* soft-argmax blur length; 1 = Huber locref loss, 0 = MSE */
    float   gamma, lengthscale, stride;   /* dgp_cfg.gamma, .lengthscale, .stride (fitdgp.py:645-647) */
    float   wn_visible, wn_hidden, locref_loss_weight;
    float   n_frames_total, n_visible_frames_total;   /* data_batcher totals (fitdgp.py:869-873) */
    int32_t use_wt, Hin, Win;             /* temporal clique (dgp_cfg.wt > 0): flow field size [nt-1, Hin, Win] */
    float   wt_max;                       /* dgp_cfg.wt_max */
} dgp_loss_desc;

int  dgp_loss_scratch_bytes(const dgp_loss_desc* d, size_t* out_bytes);
/* All pointers are device memory.  pred [nt,H,W,nj], locref_pred / locref_map / locref_mask [nt,H,W,2nj],
 * targets [n_vis_frames*nj, 2] labels in scoremap (row, col) units with NaN already replaced by 0,
 * visible_in_targets indexes rows of `targets`; S0 [nl,nj], ws / ws_max [nl].
 * Outputs: dpred, dlocref (same shapes as the predictions), mu [nt*nj,2],
 * losses[8] = {visible_loss_pred, hidden_loss_pred, visible_loss_locref, ws_loss, total_loss, total_loss_visible,
 *             wt_loss, 0}.
 * Temporal clique (use_wt; fitdgp.py:1079-1124): wt_loss = || (relu(D - wt_max) + wt_max) * w ||_F * scale with D the pixel distance of
 * a marker between consecutive frames and w the flow weight min(1 / mean flow, 1)^3 * wt_batch / H / W over the +-10 px box of the two
 * positions (bilinear crop_and_resize mean of vector_field).  The backward pass differentiates D AND w: the boxes are functions of the
 * (hidden, soft-arg-max) targets and TF's crop_and_resize has a gradient with respect to its boxes -- the weight is not a stop-gradient.
 * Any H x W (the reference's placeholders are [None, None, None, nj], fitdgp.py:1130-1142): maps up to 19 200 cells keep their Gaussian
 * target and sigmoid in LDS, larger ones recompute them where they are read -- same functions, bit-identical results. */
int  dgp_loss_fwd_bwd(const dgp_loss_desc* d, const float* pred, const float* locref_pred, const float* targets,
                      const float* locref_map, const float* locref_mask, const int32_t* visible_marker,
                      const int32_t* hidden_marker, const int32_t* visible_in_targets, const float* S0,
                      const float* ws, const float* ws_max, const float* vector_field /* [nt-1,Hin,Win] or NULL */,
                      const float* wt_batch /* [nt-1] = wt * batch_mask, or NULL */, float* dpred, float* dlocref,
                      float* mu, float* losses, void* scratch, size_t scratch_bytes, void* stream);

/* ---- DLC step-0 loss (fit_dlc: DGP/models/fitdgp.py:124; pose_net.train in DeepLabCut
 * pose_estimation_tensorflow/nnet/pose_net.py:159-190, huber_loss in nnet/losses.py:16-45):
 *   part_loss   = sum(w * sigmoid_ce(pred, part_targets)) / #nonzero(w)     (w = part_weights, NULL = all ones)
 *   locref_loss = locref_loss_weight * sum(mask * huber(locref_pred - locref_targets)) / #nonzero(mask)
 * All pointers device memory; locref_pred NULL = location_refinement off.  pred/part_* [nt,H,W,nj],
 * locref_* [nt,H,W,2nj].  Writes dpred, dlocref and losses[4] = {part_loss, locref_loss, total_loss, 0}.
 * scratch: >= 32 bytes, 8-byte aligned. */
int  dgp_dlc_loss_fwd_bwd(const float* pred, const float* locref_pred, const float* part_targets,
                          const float* part_weights, const float* locref_targets, const float* locref_mask, int32_t nt,
                          int32_t H, int32_t W, int32_t nj, float locref_loss_weight, int32_t huber, float* dpred,
                          float* dlocref, float* losses, void* scratch, size_t scratch_bytes, void* stream);

/* ---- training step (config 4): replaces sess.run([loss, train_op]) of fit_dgp / fit_dgp_labeledonly
 * (DGP/models/fitdgp.py:708-713,818; 416-418,501-505).  The trainer owns the master parameters (flat fp32 buffer
 * of every trainable TF variable: conv weights, BN gamma/beta, head weights/biases), their gradients, the momentum
 * slots and the frozen BN statistics; activations live in the caller's workspace.
 *   dgp_trainer_sync_weights : master -> forward panels, folded BN, data-gradient panels (call after every update)
 *   dgp_train_forward        : forward pass retaining activations; returns device pointers of both head outputs
 *   dgp_loss_fwd_bwd         : (above) loss and d loss / d heads
 *   dgp_train_backward       : gradients of all trainables into the flat grads buffer
 *   dgp_sgd_momentum_clip    : tf.clip_by_global_norm(clip) + MomentumOptimizer(momentum)
 *   dgp_adam_clip            : tf.clip_by_global_norm(clip) + AdamOptimizer(beta1, beta2, eps) */
typedef struct dgp_trainer dgp_trainer;
int    dgp_trainer_create(dgp_net* net, dgp_trainer** out);            /* net must have with_locref = 1 */
void   dgp_trainer_destroy(dgp_trainer* tr);
int    dgp_trainer_num_tensors(const dgp_trainer* tr, int32_t* n_tensors, int64_t* n_trainable_floats,
                               int64_t* n_stat_floats);
int    dgp_trainer_tensor_info(const dgp_trainer* tr, int32_t i, char* name, int32_t cap, int64_t* offset,
                               int64_t* size, int32_t* is_stat);
float* dgp_trainer_buffer(dgp_trainer* tr, int32_t which);  /* 0 params, 1 grads, 2 momentum, 3 BN statistics; 4: the 16-bit pass's failure flag
                                                              * (ONE int32 on the device; data-parallel runs all-reduce it with MAX before the update) */
/* Adam's state: which = 5: m, 6: v (n_trainable floats each, laid out like the parameters), 7: {beta1_power, beta2_power} as two floats.
 * They exist from the first dgp_adam_clip or the first dgp_trainer_upload into one of them (m = v = 0, powers 0.9 / 0.999 until
 * uploaded); before that dgp_trainer_buffer returns NULL for them and a download fails. */
int    dgp_trainer_upload(dgp_trainer* tr, int32_t which, int64_t offset, const float* host, int64_t n);
int    dgp_trainer_download(dgp_trainer* tr, int32_t which, int64_t offset, float* host, int64_t n);
int    dgp_trainer_workspace_bytes(const dgp_trainer* tr, int32_t nt, size_t* out_bytes);
int    dgp_trainer_sync_weights(dgp_trainer* tr, void* stream);
int    dgp_train_forward(dgp_trainer* tr, const uint8_t* frames, int32_t nt, void* workspace, size_t workspace_bytes,
                         float** scmap, float** locref, void* stream);
int    dgp_train_backward(dgp_trainer* tr, int32_t nt, void* workspace, size_t workspace_bytes, const float* dscmap,
                          const float* dlocref, void* stream);
/* (gnorm_host_or_null != NULL synchronises the stream.  After a fast / 16-bit pass the update is conditional ON THE DEVICE: a pass
 * that raised the range flag leaves parameters and momentum untouched -- see dgp_trainer_step_status.) */
int    dgp_sgd_momentum_clip(dgp_trainer* tr, float lr, float momentum, float clip_norm, float* gnorm_host_or_null,
                             void* stream);
/* TF-1's dense ApplyAdam in fp32 behind tf.clip_by_global_norm, same contract (clip_norm <= 0: no clipping; the norm goes to
 * dgp_trainer_step_status; a pass that raised the range flag leaves parameters, m, v AND the two powers untouched):
 *   g' = g * clip / max(|g|, clip);  alpha = lr sqrt(1 - beta2_power) / (1 - beta1_power)
 *   m += (g' - m)(1 - beta1);  v += (g' g' - v)(1 - beta2);  var -= alpha m / (sqrt(v) + eps);  then the powers *= beta1, beta2.
 * The powers start at beta1 / beta2 (the values of the first call) and live on the device. */
int    dgp_adam_clip(dgp_trainer* tr, float lr, float beta1, float beta2, float eps, float clip_norm, float* gnorm_host_or_null,
                     void* stream);
/* Fast pass of the training step (no reference counterpart; the step's results are the same fp32-class numbers either way).
 * dgp_trainer_fast_mode(tr, 1): the NEXT dgp_train_forward keeps the retained activations of blocks 2-4 as H2 tensors (fp16 high / low
 * cells, no fp32 twin) whose power-of-two scales are PREDICTED from the ranges the same tensors had in the previous pass (max -> [2^10,
 * 2^11): five bits of headroom), so its convs run the inference engine's cell kernels and the weight gradients read the activations in
 * place by LDS-DMA; dgp_train_backward follows what the forward did.  Ask for it only after a pass with the same frame count and
 * input size (plain or fast) -- never for the first pass after dgp_trainer_create, a weight upload or a shape change.
 * dgp_trainer_fast_status (synchronises the device): *failed != 0 -- a tensor left its predicted range (a jump of more than 2^5 up or
 * 2^7 down within one step); scoremaps, losses and gradients of that step are NOT valid: run it again with fast_mode(tr, 0) before
 * using any of them.  deepgraphpose_amd/train.py (Trainer.forward_backward) does exactly that. */
/* Precision tier of the training step (BASELINE configs[3] names bf16).  0 (default): parity -- fp32-class arithmetic, fp32 retained
 * activations.  1: the 16-bit tier -- after dgp_trainer_sync_weights, every pass requested with dgp_trainer_fast_mode(tr, 1) keeps the
 * retained activations AND the gradient tensors of blocks 2-4 as H1 cells (2 bytes per channel, scales predicted from the previous
 * step's ranges, no fp32 twins), runs their forward / data-gradient convs on one MFMA per product and reads both operands of their
 * weight gradients in place by LDS-DMA; fp32 master weights, momentum, gradient accumulation and loss; block1, the root block and the
 * heads as in tier 0.  Same protocol as the fast pass: never the first pass of a shape; dgp_trainer_fast_status reports a step whose
 * tensors left their predicted ranges (its results are invalid: run it again with fast_mode(tr, 0)).  Call dgp_trainer_sync_weights
 * after changing the tier.  A reported tier with measured gradient error, not the parity claim. */
int    dgp_trainer_set_tier(dgp_trainer* tr, int32_t tier);
int    dgp_trainer_get_tier(const dgp_trainer* tr);
/* Data-parallel training (the reference trains on one GPU; DGP/models/fitdgp.py:708-713 is the update every replica applies): the
 * gradient all-reduce of a GROUP of layers can start while dgp_train_backward is still computing the earlier layers.  Group k = floats
 * [lo[k], hi[k]) of the flat gradient buffer (dgp_trainer_buffer(tr, 1)), in the order the LAST backward pass completes them (heads and
 * last bottleneck units first, stem last; the groups tile the buffer; *n_groups = 0 before the first pass).
 * dgp_trainer_grad_group_wait makes `stream` wait for group k (hipStreamWaitEvent: nothing blocks on the host). */
int    dgp_trainer_grad_groups(dgp_trainer* tr, int32_t max_groups, int32_t* n_groups, int64_t* lo, int64_t* hi);
int    dgp_trainer_grad_group_wait(dgp_trainer* tr, int32_t k, void* stream);
int    dgp_trainer_fast_mode(dgp_trainer* tr, int32_t enable);
int    dgp_trainer_fast_status(dgp_trainer* tr, int32_t* was_fast, int32_t* failed);
/* ONE synchronisation per training step: enqueue forward, loss, backward, dgp_sgd_momentum_clip(..., NULL gnorm, ...) and
 * dgp_trainer_sync_weights on `stream` without reading anything back, then call this -- a last tiny kernel writes the n_losses (<= 8)
 * device floats at d_losses (dgp_loss_fwd_bwd's `losses`; NULL / 0: none), the gradient norm the optimiser saw and the pass status into
 * pinned host memory, and the call waits for the stream once.  After a fast / 16-bit pass whose tensors left their predicted ranges
 * (*failed != 0) the momentum kernel has SKIPPED its update on the device (it reads the flag), so the step can be run again on the
 * parity path as if nothing had happened.  Replaces the read-backs of sess.run([loss, train_op]) (DGP/models/fitdgp.py:818). */
int    dgp_trainer_step_status(dgp_trainer* tr, const float* d_losses, int32_t n_losses, float* losses, float* gnorm,
                               int32_t* was_fast, int32_t* failed, void* stream);

/* ---- single-layer entry points (used by the parity tests and by fit_dgp later) ---- */

/* slim.conv2d / conv2d_same semantics on NHWC fp32 with HWIO weights supplied packed by
 * dgp_pack_conv_weights.  y = relu?( conv(x) * scale + bias (+ residual) ). */
typedef struct dgp_conv_desc {
    int32_t N, H, W, Cin;          /* input  (Cin % 4 == 0) */
    int32_t Cout;                  /* real output channels */
    int32_t KH, KW, stride, rate;
    int32_t pad_t, pad_l;          /* zero padding before (TF SAME / conv2d_same) */
    int32_t Ho, Wo;                /* output spatial size */
    int32_t relu;                  /* 1: apply ReLU */
    int32_t res_stride;            /* 0: no residual; s>=1: residual[n, ho*s, wo*s, :] */
    int32_t res_H, res_W;          /* residual spatial size */
} dgp_conv_desc;

size_t dgp_packed_weight_floats(int32_t KH, int32_t KW, int32_t Cin, int32_t Cout);
/* host -> host repack: HWIO [KH,KW,Cin,Cout] -> k-chunked panels [Kp/4][CoutP][4] */
int  dgp_pack_conv_weights(const float* hwio, int32_t KH, int32_t KW, int32_t Cin,
                           int32_t Cout, float* packed);
int  dgp_conv2d(const dgp_conv_desc* d, const float* x, const float* packed_w,
                const float* scale /*[Cout] or NULL*/, const float* bias /*[Cout] or NULL*/,
                const float* residual, float* y, void* stream);
/* Same, with the operand ranges the fp16-split kernels need.  A range is a device array of DGP_ABSMAX_SLOTS floats
 * whose maximum is (an upper bound of) max |tensor| (producers spread their atomics over the slots); fill one with
 * dgp_tensor_absmax.  With x_absmax and w_absmax present the fp16 high/low split (3 MFMAs per fp32-class product)
 * may be used, otherwise the bf16 3-way split (6 MFMAs, no range requirement).  y_absmax (zero it first; may be
 * NULL) receives max |y| so that y can feed the next ranged call. */
#define DGP_ABSMAX_SLOTS 256
int  dgp_conv2d_ranged(const dgp_conv_desc* d, const float* x, const float* packed_w, const float* scale, const float* bias,
                       const float* residual, float* y, const float* x_absmax, const float* w_absmax, float* y_absmax,
                       void* stream);
/* Same, with room for the grid-tail K-split (plan_tail_ksplit in csrc/dgp_conv_split.hip: the tiles of an underfull last round split
 * their K range over up to 4 workgroups, raw partial sums go to the slab, a fix-up launch sums them in fixed order).  tail_slab: the
 * caller's device memory, tail_slab_bytes < 4 GiB (DGP_ERR_INVALID otherwise); nothing is allocated.  NULL / 0: dgp_conv2d_ranged. */
int  dgp_conv2d_ranged_slab(const dgp_conv_desc* d, const float* x, const float* packed_w, const float* scale, const float* bias,
                            const float* residual, float* y, const float* x_absmax, const float* w_absmax, float* y_absmax,
                            float* tail_slab, size_t tail_slab_bytes, void* stream);
/* What the launch layer would run for a layer: the host-side plan of dgp_conv2d_ranged (in_fmt 0), dgp_conv2d_h2 (in_fmt 1) or
 * dgp_conv2d_h1 (in_fmt 2), without launching anything.  Formats: 0 fp32, 1 H2, 2 H1.  have_ranges: x_absmax and w_absmax are given
 * (cell inputs always have them); have_cells: the weight panel also exists as fp16 cells (always with cell inputs; DGP_CONV2D_CELLS=1
 * for dgp_conv2d_ranged); slab_bytes: the tail slab's size (0: none).  force_tile: a tile id, -1: the launch's own choice.  n_cu: the
 * number of compute units to plan for, 0: the current device's; with n_cu > 0 no GPU is needed.  A launch the kernels refuse returns
 * the error the launch would return. */
typedef struct dgp_conv_plan {
    int32_t tile;                    /* tile id after the launch's fall-backs */
    int32_t family;                  /* 0 fp32 MFMA, 1 fp32 loader-specialised, 2 split (bf16 / fp16) */
    int32_t mode, cs, dma, deep;     /* split family: loader walk (0 run time, 1 per tap, 2 pointwise, 3 halo ring), compute-side split,
                                        LDS-DMA loaders, deep DMA ring */
    int32_t ah2, oh2, h1;            /* input in cells, output in cells, the cells are H1 */
    int32_t lds;                     /* dynamic LDS bytes */
    int32_t mtiles, ntiles, grid;    /* row tiles, column tiles, workgroups of the main launch */
    int32_t tail_ksplit, n_main;     /* K-split of the grid's tail (0: none): workgroups per tail tile, tiles in front of the tail */
    int32_t st_gn, st_mc, st_mb;     /* supertile order (st_gn 0: plain): column tiles per group, row tiles per chunk and per band */
    int32_t n_cu;                    /* compute units planned for */
    char    kernel_name[32];
    int32_t w22;                     /* split family, cell inputs: 1 = 2 x 2 compute waves of 64 x 64, 0 = 4 x 1 of 32 x 128 (DGP_WAVE_2X2) */
} dgp_conv_plan;
int  dgp_conv2d_plan(const dgp_conv_desc* d, int32_t in_fmt, int32_t out_fmt, int32_t res_fmt, int32_t have_ranges, int32_t have_cells,
                     size_t slab_bytes, int32_t force_tile, int32_t n_cu, dgp_conv_plan* out);
/* ---- single-layer BACKWARD entry points: the launchers dgp_train_backward uses, exposed so that the weight-gradient and
 * data-gradient kernels can be checked layer by layer at the real shapes (no reference counterpart: TF differentiates the graph,
 * DGP/models/fitdgp.py:708-713).  `d` always describes the FORWARD conv x [N,H,W,Cin] -> y [N,Ho,Wo,Cout].
 *   dgp_conv2d_wgrad : dw_raw[(kh, kw, ci)][co] = sum over output pixels of x[...] * dy[...] (HWIO order, overwritten) and
 *                      colsum[co] = sum dy[.., co] (2 * Cout floats, second half scratch; may be NULL).  With both operand ranges
 *                      (DGP_ABSMAX_SLOTS floats each) and a tile of 128 x 128 the fp16-split kernel runs, else fp32 MFMA.
 *   dgp_conv2d_dgrad : dx = gate(convT(dy; w * scale) + dx_add); w_hwio device HWIO weights; scale [Cout] or NULL; mask [N,H,W,Cin]
 *                      or NULL (gate: mask > 0); dx_add NULL, or a gradient on dx's grid (add_mode 1) or on the 2x coarser grid
 *                      (add_mode -2, the subsample shortcut).  scratch: dgp_conv2d_dgrad_scratch_bytes(d) device bytes.
 *                      Cout % 32 == 0, Cin % 4 == 0; ranged bit 1 (the gate is an H2 tensor): bit 0, a mask, Cin % 8 == 0 and Cin >= 64. */
int    dgp_conv2d_wgrad(const dgp_conv_desc* d, const float* x, const float* dy, const float* x_absmax, const float* dy_absmax,
                        float* dw_raw, float* colsum, void* stream);
/* dgp_conv2d_wgrad on the LDS-DMA tile of the training step (csrc/dgp_wgrad.hip, wgrad_dma).  Inside dgp_train_backward both operands
 * of a 128 x 128 weight-gradient tile also exist as fp16 high / low cells (the H2 layout below), written by their producers' epilogues
 * with a power-of-two scale PREDICTED from the range the same tensor had one step earlier (max -> [2^10, 2^11)); the kernel moves the
 * cells by LDS-DMA (no split arithmetic, no register staging) and checks this step's ranges against the predicted scales: outside
 * [2^4, 65000) after scaling -- first step, a jump of more than 2^5 -- the workgroup computes its tile from the fp32 tensors on the
 * fp32 matrix pipe instead.  This entry point makes the copies itself from x / dy and the given "previous" ranges, so that the tile
 * and both of its paths can be checked layer by layer.  scratch: 4 * (numel(x) + numel(dy)) device bytes; x_absmax / dy_absmax /
 * x_prev / dy_prev: DGP_ABSMAX_SLOTS floats each; Cin = 16 * 2^k, Cout % 8 == 0, KH * KW * Cin >= 128, Cout >= 128. */
int    dgp_conv2d_wgrad_shadow(const dgp_conv_desc* d, const float* x, const float* dy, const float* x_absmax, const float* dy_absmax,
                               const float* x_prev, const float* dy_prev, void* scratch, float* dw_raw, float* colsum, void* stream);
size_t dgp_conv2d_dgrad_scratch_bytes(const dgp_conv_desc* d);
int    dgp_conv2d_dgrad(const dgp_conv_desc* d, const float* dy, const float* w_hwio, const float* scale, const float* mask,
                        const float* dx_add, int32_t add_mode, float* dx, void* scratch, int32_t ranged, void* stream);
/* ---- the same for the 16-bit tier (dgp_trainer_set_tier(tr, 1)), whose backward pass runs other kernels: every tensor is an H1 tensor
 * (below) whose scale is PREDICTED from the range slots the same tensor had one step earlier -- max = m 2^E (1 <= m < 2) -> scale
 * 2^(10 - E), no scale (nothing written) for a zero or non-finite maximum; usable while this step's maximum times the scale stays in
 * [16, 65000).  These entry points take fp32 tensors plus such "previous step" slots (DGP_ABSMAX_SLOTS floats each), make the H1
 * tensors with the trainer's own converter, leave them in `scratch` for the caller to read, and run the launchers of the 16-bit pass.
 * No reference counterpart (the reference computes in fp32).  `d` describes the FORWARD conv. */
/* H1 cells written with the scale `prev` predicts -> fp32; gate_h1: an H1 tensor of the same shape (out = 0 where its half is not
 * positive) or NULL.  The converter the 16-bit pass uses where a gradient leaves the H1 units. */
int    dgp_h1_to_f32_pred(const void* x_h1, size_t n_halves, const float* prev, const void* gate_h1, float* out, void* stream);
/* dgp_conv2d_wgrad on wgrad_dma_h1: both operands H1 tensors read in place by LDS-DMA, one fp16 MFMA per product, the 128-column tile
 * partly filled for narrower layers.  scratch: [x as H1 | dy as H1], 2 * (numel(x) + numel(dy)) bytes.  *flag (device int32): zeroed, then
 * 2 when a tensor left its predicted range -- dw_raw / colsum are zero then: this kernel has no fp32 path behind it.
 * Cin = 16 * 2^k, Cout % 8 == 0. */
int    dgp_conv2d_wgrad_h1(const dgp_conv_desc* d, const float* x, const float* dy, const float* x_absmax, const float* dy_absmax,
                           const float* x_prev, const float* dy_prev, void* scratch, float* dw_raw, float* colsum, int32_t* flag, void* stream);
/* dgp_conv2d_dgrad as the H1 -> H1 launch of the 16-bit pass: dx_h1 (halves, [N,H,W,Cin]) = fp16(gate(convT(dy; w * scale) + dx_add) * the
 * scale dx_prev predicts).  The panel comes from the same pack as dgp_conv2d_dgrad, as high-only fp16 cells; dy and dx_add are converted
 * with dy_prev / add_prev; gate_h1 is the gate ALREADY as H1 cells (dgp_f32_to_h1, any scale: only its sign is read) or NULL; a stride-2
 * layer reads dy from a zero-stuffed H1 copy on the 2 Ho x 2 Wo grid through a stride-1 launch, as the pass does.
 * scratch: dgp_conv2d_dgrad_scratch_bytes(d) bytes, then [dy as H1: 2 numel(dy)][dx_add as H1: 2 numel(dx_add)][stride 2: 8 numel(dy)].
 * *flag (device int32, may be NULL): zeroed, then odd when dx left the range dx_prev predicts.  Cin % 64 == 0, Cout % 64 == 0. */
int    dgp_conv2d_dgrad_h1(const dgp_conv_desc* d, const float* dy, const float* w_hwio, const float* scale, const void* gate_h1,
                           const float* dx_add, int32_t add_mode, const float* dy_prev, const float* dx_prev, const float* add_prev,
                           void* scratch, void* dx_h1, int32_t* flag, void* stream);
/* The stem's weight gradient with the max-pool's backward fused in (stem_wgrad_h1_kernel + stem_wgrad_reduce_kernel): x_centred
 * [B,H,W,4] fp32, dpool [B,HP,WP,64] fp32 (converted with dpool_prev), idx [B,HP,WP,64] bytes: position a * 3 + b of each pool window's
 * FIRST maximum (row-major, window origin 2 q - pad), H1 = ceil(H / 2), HP = ceil(H1 / 2) (same for W).  dw [49 * 4][64], colsum [64].
 * scratch: 2 * numel(dpool) bytes rounded up to 256, then B * ceil(H1 / 4) * ceil(W1 / 32) rows of (196 * 64 + 64) floats. */
int    dgp_stem_wgrad_h1(const float* x_centred, const float* dpool, const float* dpool_prev, const uint8_t* idx, int32_t B, int32_t H,
                         int32_t W, int32_t H1, int32_t W1, int32_t HP, int32_t WP, void* scratch, float* dw, float* colsum, void* stream);
/* ---- the root block's max-pool (3x3 / 2, SAME) with its first-maximum record, and the fused root block, as layers.  Maps: H1 = ceil(H / 2),
 * HP = ceil(H1 / 2) (same for W); anything else is DGP_ERR_INVALID.  The record idx [B,HP,WP,64] holds per window and channel the position
 * a * 3 + b (row-major from the window origin 2 q - pad) of its FIRST maximum under `>`.  Two conventions for windows that hold nothing
 * positive: the unfused pool records the first VALID position whatever the values are; the fused root block records 0. */
/* The training step's unfused pool (maxpool_fwd_idx_kernel): c1 [B,H1,W1,64] fp32 -> pool [B,HP,WP,64] fp32 + idx; prev and pool_h1 both
 * set: also the H1 copy fp16(pool * the scale prev predicts) (halves [B,HP,WP,64]; nothing is written when prev predicts no scale). */
int    dgp_maxpool_fwd_idx(const float* c1, int32_t B, int32_t H1, int32_t W1, int32_t HP, int32_t WP, const float* prev, float* pool,
                           uint8_t* idx, void* pool_h1, void* stream);
/* Its backward (maxpool_bwd_idx_kernel): dc1 [B,H1,W1,64] = (c1 > 0) * sum of dpool over the windows whose record names the pixel, windows
 * added in ascending (row, column) order in fp32; c1 == NULL: no gate (the 16-bit tier).  A record that names a position outside the map
 * routes that window's gradient nowhere. */
int    dgp_maxpool_bwd_idx(const float* c1, const float* dpool, const uint8_t* idx, int32_t B, int32_t H1, int32_t W1, int32_t HP, int32_t WP,
                           float* dc1, void* stream);
/* The fused root block (stem_pool_fused_kernel) on its own: frames [B,H,W,3] bytes at any byte alignment, w_hwio [7,7,3,64], bn_scale /
 * bn_bias [64] (device), mean_pixel [3] (HOST) -> out [B,HP,WP,64] as cells: cells 1 = H2 (fp32-sized, the parity tier's inference
 * instantiation), 2 = H1 (halves, the 16-bit tier's).  The weight cells are built as dgp_trainer_sync_weights builds them.  Scale: 2^out_exp,
 * or with out_prev (cells 2 only) the one those range slots predict, as the training step launches it; idx (cells 2 with out_prev only;
 * DGP_ERR_STATE without out_prev): the first-maximum record.  out_absmax [DGP_ABSMAX_SLOTS]: zeroed, then the tracked range of the output.
 * A batch of 2^31 bytes or more is DGP_ERR_INVALID.  scratch: dgp_root_block_scratch_bytes() device bytes. */
size_t dgp_root_block_scratch_bytes(void);
int    dgp_root_block(const uint8_t* frames, int32_t B, int32_t H, int32_t W, const float* w_hwio, const float* bn_scale, const float* bn_bias,
                      const float* mean_pixel, int32_t cells, int32_t out_exp, const float* out_prev, uint8_t* idx, void* scratch, void* out,
                      float* out_absmax, void* stream);
/* Both heads' backward of the 16-bit pass on one stream: feat [N,h,w,Cin] (converted with feat_prev), dscmap [N,2h,2w,nj] and dlocref
 * [N,2h,2w,2nj] gathered phase-major into ONE H1 tensor of CT columns with one scale (dph_prev), w_part / w_locref in the trainer's
 * layout [3,3,njt,Cin]; one weight-gradient launch, two finalisations (dw_* [3,3,njt,Cin], db_* [njt]), one 2x2-tap data gradient
 * dfeat_h1 (halves, scale from dfeat_prev, gated by feat).  DGP_ERR_INVALID for head widths the merged panel does not take.
 * scratch, each part rounded up to 256 bytes: [feat H1: 2 N h w Cin][merged gradient H1: 2 N h w CT][panel: 16 CT Cin][its cells:
 * 8 CT Cin][dwraw: 16 Cin CT][colsum: 8 CT][4 range slots] with CT = the merged tensor's columns (next_pow2(4 nj) + next_pow2(8 nj), rounded up to a multiple of 64);
 * 2 N h w (Cin + CT) + 48 Cin CT + 16384 bytes suffice for Cin % 128 == 0.  *flag as dgp_conv2d_wgrad_h1. */
int    dgp_heads_backward_h1(const float* feat, const float* feat_prev, const float* dscmap, const float* dlocref, const float* dph_prev,
                             const float* w_part, const float* w_locref, const float* dfeat_prev, int32_t N, int32_t h, int32_t w,
                             int32_t Cin, int32_t nj, void* scratch, float* dw_part, float* db_part, float* dw_locref, float* db_locref,
                             void* dfeat_h1, int32_t* flag, void* stream);
/* ---- "H2" activation format.  Inside dgp_forward / dgp_infer every tensor from the pool output to the block4 features lives
 * in HBM as fp16 high / low cell pairs: per pixel and 8 channels [8 halves hi | 8 halves lo] = 32 bytes (the footprint and the
 * addresses of 8 fp32 channels) holding x * 2^exp, hi = fp16(x 2^exp), lo = fp16(x 2^exp - hi): 22 significant bits.  The
 * producing conv splits once in its epilogue; the consuming conv's K loop copies the cells into the MFMA operand image and only
 * issues ds_read + MFMA.  exp is per tensor, calibrated by the FIRST forward after dgp_net_load_weights (layer by layer, with
 * hidden stream syncs: max |tensor| * 2^exp lands in [2^10, 2^11), 4 bits under the fp16 limit) and frozen afterwards, so the
 * results are a deterministic function of the frames and the scales.  Every forward checks the tracked ranges against the scales
 * on the device; dgp_net_range_status reports (and clears) an overflow -- the results of a forward that overflowed are invalid,
 * the next forward re-calibrates on its own batch and the caller re-runs what it needs.  DGP_H2=0 keeps fp32 activations.
 * The entry points below expose the format for tests and for features handed out at the boundary. */
int  dgp_f32_to_h2(const float* x, size_t n_floats, int32_t scale_exp, void* out, void* stream);
int  dgp_h2_to_f32(const void* x, size_t n_floats, int32_t scale_exp, float* out, void* stream);
/* dgp_conv2d on H2 tensors: x (H2, exponent x_exp) -> y (H2 with y_exp, or fp32 when y_is_h2 == 0); residual fp32 or H2.
 * w_absmax: range slots of packed_w (dgp_tensor_absmax); cells_scratch: >= dgp_packed_weight_floats(...) * 4 device bytes.
 * fp32 output exists for 1x1 / stride-1 layers only (the heads' pointwise GEMM) and takes an fp32 residual; every other combination
 * with y_is_h2 == 0, and an H2 residual with an fp32 output, returns DGP_ERR_INVALID. */
int  dgp_conv2d_h2(const dgp_conv_desc* d, const void* x_h2, int32_t x_exp, const float* packed_w, const float* w_absmax,
                   const float* scale, const float* bias, const void* residual, int32_t res_is_h2, int32_t res_exp, void* y,
                   int32_t y_is_h2, int32_t y_exp, float* y_absmax, void* cells_scratch, void* stream);
/* dgp_conv2d_h2 with room for the grid-tail K-split (see dgp_conv2d_ranged_slab; cell inputs split only under DGP_TAIL_SPLIT=2) */
int  dgp_conv2d_h2_slab(const dgp_conv_desc* d, const void* x_h2, int32_t x_exp, const float* packed_w, const float* w_absmax,
                        const float* scale, const float* bias, const void* residual, int32_t res_is_h2, int32_t res_exp, void* y,
                        int32_t y_is_h2, int32_t y_exp, float* y_absmax, void* cells_scratch, float* tail_slab, size_t tail_slab_bytes,
                        void* stream);
/* ---- "H1" activation format: the 16-bit tier.  dgp_net_set_tier(net, 1) makes dgp_forward / dgp_infer keep every tensor from the pool
 * output to the block4 features as ONE 16-byte cell of 8 halves per pixel and 8 channels -- fp16(x * 2^exp), bit for bit the high cell
 * of the H2 pair: plain NHWC fp16 with the same calibrated per-tensor scales -- and multiply them with fp16 weights on one MFMA per
 * product (fp32 accumulation, fp32 epilogue arithmetic, fp32 heads and soft-argmax).  Half the activation bytes and a third of the
 * matrix work of the parity tier (tier 0, the default); 11-bit operands, so NOT inside the 1e-3 px gate: a reported tier with measured
 * error (bench.py `tier_f16`), never the parity claim.  No reference counterpart (the reference computes in fp32 on TF-1.x).
 * Switching tiers re-calibrates on the next forward.  DGP_CONV_MODE=f16 in the environment makes tier 1 the default of new nets. */
int  dgp_net_set_tier(dgp_net* net, int32_t tier);
int  dgp_net_get_tier(const dgp_net* net);
int  dgp_f32_to_h1(const float* x, size_t n_floats, int32_t scale_exp, void* out, void* stream);
int  dgp_h1_to_f32(const void* x, size_t n_floats, int32_t scale_exp, float* out, void* stream);
/* dgp_conv2d on H1 tensors (layer tests): x (H1, exponent x_exp; Cin % 64 == 0) -> y (H1 with y_exp, or fp32 when y_is_h1 == 0: 1x1 /
 * stride-1 layers only, no residual); residual_h1: an H1 tensor on y's grid (d->res_stride) or NULL.  cells_scratch:
 * >= dgp_packed_weight_floats(...) * 2 device bytes. */
int  dgp_conv2d_h1(const dgp_conv_desc* d, const void* x_h1, int32_t x_exp, const float* packed_w, const float* w_absmax,
                   const float* scale, const float* bias, const void* residual_h1, int32_t res_exp, void* y,
                   int32_t y_is_h1, int32_t y_exp, float* y_absmax, void* cells_scratch, void* stream);
/* The engine's chain kernel at layer level (tests): conv3 of a bottleneck unit + shortcut + ReLU (X', written once) and conv1 of the
 * NEXT unit (R1') in one launch; conv1 takes X' from the accumulator registers, so the 4C-wide tensor is not re-read.  Replaces two
 * slim.conv2d calls of consecutive `bottleneck` units (PET/nnet/pose_net.py:46-52 -> slim resnet_v1.bottleneck: conv3 without
 * activation, relu(shortcut + residual), then conv1 of the next unit).  All device tensors H2 with the given exponents; weights
 * (row-major [K][N], K = C (+ CIN2 rows of the BN-folded shortcut conv), N = 4 C; w1 [4 C][C1]) and BN affines are HOST arrays.
 * res_mode: 0 K-concatenated shortcut conv (src2 = its input [M][CIN2], same exponent as r2), 1 identity (src2 = X [M][4C]),
 * 2 subsample of a stride-2 unit (src2 = X [N, res_H, res_W, 4C], read at (2 ho, 2 wo)).  DGP_ERR_INVALID when no kernel instance
 * exists for the shape.  Synchronises the stream (per-call weight packing). */
int  dgp_chain_h2(int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t C1, int32_t CIN2, int32_t res_mode, int32_t res_H, int32_t res_W,
                  const void* r2_h2, int32_t r2_exp, const void* src2_h2, int32_t src2_exp,
                  const float* w3cat, const float* scale3, const float* bias3, const float* w1, const float* scale1, const float* bias1,
                  void* xout_h2, int32_t xout_exp, void* r1_h2, int32_t r1_exp, float* xout_absmax, float* r1_absmax, void* stream);
/* The engine's unit kernel at layer level (tests; block1 shapes, C = 64): additionally conv2 (3x3, stride 1, SAME, BN, ReLU) of the
 * unit in front -- slim `bottleneck`'s conv2 -> conv3 -> add -> relu and the next unit's conv1 in ONE launch.  r1 [N, H, W, C] is
 * conv2's input (read with a one-pixel halo: r1out must be another buffer); R2 exists only in registers (r2_exp: the scale its fp16
 * fragments are split with; its range is tracked into r2_absmax).  w2: HWIO [3][3][C][C] host array.  Other arguments as dgp_chain_h2. */
int  dgp_unit_h2(int32_t N, int32_t H, int32_t W, int32_t C, int32_t C1, int32_t CIN2, int32_t res_mode,
                 const void* r1_h2, int32_t r1_exp, const void* src2_h2, int32_t src2_exp,
                 const float* w2, const float* scale2, const float* bias2, int32_t r2_exp,
                 const float* w3cat, const float* scale3, const float* bias3, const float* w1, const float* scale1, const float* bias1,
                 void* xout_h2, int32_t xout_exp, void* r1out_h2, int32_t r1out_exp, float* r2_absmax, float* xout_absmax, float* r1_absmax,
                 void* stream);
/* dgp_chain_h2 / dgp_unit_h2 on H1 tensors (the 16-bit tier's instances of the same kernels: 2 bytes per channel, the chunks' high weight
 * fragments only, one MFMA per product; a REPORTED tier, see dgp_net_set_tier).  Same arguments, every device tensor H1. */
int  dgp_chain_h1(int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t C1, int32_t CIN2, int32_t res_mode, int32_t res_H, int32_t res_W,
                  const void* r2_h1, int32_t r2_exp, const void* src2_h1, int32_t src2_exp,
                  const float* w3cat, const float* scale3, const float* bias3, const float* w1, const float* scale1, const float* bias1,
                  void* xout_h1, int32_t xout_exp, void* r1_h1, int32_t r1_exp, float* xout_absmax, float* r1_absmax, void* stream);
int  dgp_unit_h1(int32_t N, int32_t H, int32_t W, int32_t C, int32_t C1, int32_t CIN2, int32_t res_mode,
                 const void* r1_h1, int32_t r1_exp, const void* src2_h1, int32_t src2_exp,
                 const float* w2, const float* scale2, const float* bias2, int32_t r2_exp,
                 const float* w3cat, const float* scale3, const float* bias3, const float* w1, const float* scale1, const float* bias1,
                 void* xout_h1, int32_t xout_exp, void* r1out_h1, int32_t r1out_exp, float* r2_absmax, float* xout_absmax, float* r1_absmax,
                 void* stream);
/* The same launches with the X' keep stride (tests).  slim's resnet_v1 puts a block's stride on its last unit, whose shortcut is
 * subsample(x, 2) = x[:, ::2, ::2]; the engine's launch in front of such a unit already computes that unit's conv1, so X' is read at
 * even rows and columns only and the engine stores only those (DGP_XOUT_SUBSAMPLE).  xout_keep 1: all of xout is written, as by the
 * entry points above; 2: only pixels (y, x) with y and x even -- the other pixels of xout keep the bytes they held.  r1 and all range
 * slots (xout_absmax included) cover every pixel either way.  Any other xout_keep: DGP_ERR_INVALID.  h1 != 0: every device tensor is H1
 * (dgp_chain_h1 / dgp_unit_h1), else H2.  Other arguments as dgp_chain_h2 / dgp_unit_h2. */
int  dgp_chain_xkeep(int32_t h1, int32_t xout_keep, int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t C1, int32_t CIN2, int32_t res_mode,
                     int32_t res_H, int32_t res_W, const void* r2, int32_t r2_exp, const void* src2, int32_t src2_exp,
                     const float* w3cat, const float* scale3, const float* bias3, const float* w1, const float* scale1, const float* bias1,
                     void* xout, int32_t xout_exp, void* r1, int32_t r1_exp, float* xout_absmax, float* r1_absmax, void* stream);
int  dgp_unit_xkeep(int32_t h1, int32_t xout_keep, int32_t N, int32_t H, int32_t W, int32_t C, int32_t C1, int32_t CIN2, int32_t res_mode,
                    const void* r1, int32_t r1_exp, const void* src2, int32_t src2_exp,
                    const float* w2, const float* scale2, const float* bias2, int32_t r2_exp,
                    const float* w3cat, const float* scale3, const float* bias3, const float* w1, const float* scale1, const float* bias1,
                    void* xout, int32_t xout_exp, void* r1out, int32_t r1out_exp, float* r2_absmax, float* xout_absmax, float* r1_absmax,
                    void* stream);
/* Synchronises `stream`, then: *overflow = 1 if any forward since the last call outgrew a calibrated scale (the flag is cleared
 * and the net re-calibrates on its next forward); *calibrations = calibration passes run so far. */
int  dgp_net_range_status(dgp_net* net, int32_t* overflow, int32_t* calibrations, void* stream);
int  dgp_net_recalibrate(dgp_net* net);      /* force a calibration pass on the next forward */
/* What dgp_net_range_status does to the engine when it reports an overflow (re-calibrate on the next forward with 3 more bits of
 * headroom), for a rank that did not overflow itself but must follow one that did (sharded runs stay bit-identical). */
int  dgp_net_widen(dgp_net* net);
/* Back to the state right after dgp_net_load_weights as far as the activation scales go: default headroom, calibration pass on the next
 * forward.  For an engine that is kept between videos (models/eval.py, the session kept by setup_dgp_eval_graph): the next video's first
 * batch then sets the same scales -- and every later frame gets the same bits -- as on a freshly built engine. */
int  dgp_net_reset_scales(dgp_net* net);
/* The calibrated activation scales of `src` (same network, weights, tier and frame size) become `dst`'s: what `dst` would have found by
 * calibrating on the same batch itself -- the calibration is deterministic -- without its layer-by-layer pass.  For callers that keep
 * several engines in step (two batches in flight: one engine calibrates on the video's first batch, the others copy).  Synchronises
 * `stream` (the stream `dst` runs on). */
int  dgp_net_copy_scales(dgp_net* dst, const dgp_net* src, void* stream);

/* slots = max(slots, max |x[0..n)|) on the device (zero the DGP_ABSMAX_SLOTS floats before the first call). */
int  dgp_tensor_absmax(const float* x, size_t n, float* absmax_dev, void* stream);
int  dgp_maxpool_3x3s2_same(const float* x, int32_t N, int32_t H, int32_t W, int32_t C,
                            float* y, void* stream);
int  dgp_preprocess_u8(const uint8_t* frames, int64_t n_pixels, const float mean[3],
                       float* out_nhwc4, void* stream);
/* Motion energy of a uint8 frame sequence on the device (replaces the per-frame numpy loop of calculate_motion_energy,
 * DGP/dataset.py:29-43).  sums[t] = sum over the frame's bytes of (frames[t] - frames[t-1]) mod 256 -- the
 * reference subtracts uint8 arrays, so the difference wraps -- for t >= 1, and for t = 0 against prev_frame (the last frame of
 * the previous chunk; NULL: sums[0] = 0).  The reference's value is sums[t] / frame_bytes in float64 (exact).  frames:
 * [n_frames][frame_bytes] device bytes; sums: n_frames device uint64 (overwritten).  Integer sums, bit-exact, order-independent. */
int  dgp_motion_energy(const uint8_t* frames, int64_t frame_bytes, int32_t n_frames, const uint8_t* prev_frame,
                       uint64_t* sums, void* stream);

/* ---- Farneback optical flow (replaces cv2.calcOpticalFlowFarneback in learn_wt, DGP/models/fitdgp_util.py:454-467, called from
 * DGP/models/fitdgp.py:771-775: the flow magnitude the temporal clique reads as vector_field).  Parameters as OpenCV's
 * calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags); the reference uses
 * (0.5, 3, 15, 3, 5, 1.2, 0).  Rules: 0 < pyr_scale < 1, levels >= 0, winsize odd 3..31, iterations >= 1, poly_n 5 | 7,
 * poly_sigma > 0, flags 0 (no Gaussian window, no initial flow), frames >= 16 x 16, n_frames >= 2; anything else is DGP_ERR_INVALID. */
typedef struct dgp_flow_params {
    double  pyr_scale;
    int32_t levels, winsize, iterations, poly_n;
    double  poly_sigma;
    int32_t flags;
} dgp_flow_params;

/* Host only (no GPU): validates the parameters and gives the device scratch dgp_optical_flow needs for n_frames frames of H x W, and
 * the pyramid levels it builds (levels clamped as OpenCV does: a level narrower or lower than 32 pixels is not built).
 * Reference call site: DGP/models/fitdgp_util.py:454-467. */
int  dgp_optical_flow_scratch_bytes(int32_t n_frames, int32_t H, int32_t W, const dgp_flow_params* p, size_t* bytes,
                                    int32_t* levels_used);
/* Flow of the n_frames - 1 consecutive pairs of a uint8 BGR frame sequence (channel 0 = B: the reference's COLOR_BGR2GRAY), all pairs
 * in every launch.  frames: device [n_frames][H][W][3]; flow: device fp32 [n_frames-1][H][W][2] (dx, dy) or NULL; magnitude: device
 * fp32 [n_frames-1][H][W] = |dx| + |dy| (learn_wt's np.abs(flow).sum(2), dgp_loss_fwd_bwd's vector_field layout) or NULL; at least
 * one of the two.  scratch: dgp_optical_flow_scratch_bytes device bytes.  fp32, no atomics: bit-identical from run to run.
 * Reference call site: DGP/models/fitdgp_util.py:454-467. */
int  dgp_optical_flow(const uint8_t* frames, int32_t n_frames, int32_t H, int32_t W, const dgp_flow_params* p, float* flow,
                      float* magnitude, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Resize + crop of uint8 RGB frames, bit-exact with Pillow (replaces the per-frame PIL.Image.resize + .crop of estimate_pose,
 * DGP/models/eval.py:307-326).  The contract is Pillow's ImagingResample at 8 bits per channel with the BICUBIC filter -- what
 * Image.resize(size=...) runs by default.  Per axis, in_size -> out_size, PRECISION_BITS = 22:
 *   scale = in / out, filterscale = max(scale, 1), support = 2 * filterscale, ksize = (int)ceil(support) * 2 + 1;
 *   output xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
 *              n = min((int)(center + support + 0.5), in) - xmin, w[x] = bicubic((x + xmin - center + 0.5) / filterscale), a = -0.5,
 *              divided by their left-to-right sum, in double; k[x] = (int)(w * 2^22 +- 0.5), rounded away from zero;
 *   a pass is clip((2^21 + sum k[x] * pixel[xmin + x]) >> 22, 0, 255) on int32.  The horizontal pass runs first and its result is clipped
 *   to uint8 before the vertical pass.  crop(left, upper, right, lower) selects that box of the resized image; what lies outside is 0. */

/* Host only (no GPU): the table width of one axis.  Non-positive sizes (or sizes above 2^24) are DGP_ERR_INVALID. */
int  dgp_resize_plan_size(int32_t in_size, int32_t out_size, int32_t* ksize);
/* Host only (no GPU): one axis' tables.  bounds: int32 [out_size][2] = (xmin, n); coeffs: int32 [out_size][ksize], zero-padded past n.
 * Double arithmetic in Pillow's operation order with contraction off: the integers are Pillow's. */
int  dgp_resize_plan(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs);
/* src: device uint8 [B][H][W][3] -> resized to RH x RW -> box (left, upper, right, lower; host int32[4], NULL = the whole resized
 * image) -> dst: device uint8 [B][OH][OW][3], OH = lower - upper, OW = right - left (RH, RW without a box).  Only the box is computed;
 * its parts outside the resized image are written as zeros.  d_plan_x (W -> RW) and d_plan_y (H -> RH): device int32 arrays holding
 * dgp_resize_plan's bounds followed by its coeffs ([out][2] then [out][ksize]); ksize_x / ksize_y: dgp_resize_plan_size's.  One launch,
 * integer arithmetic, no atomics, no scratch: bit-identical from run to run.  A horizontal reduction whose row segment for 64 output
 * pixels does not fit the kernel's LDS (about 20 x) is DGP_ERR_INVALID before anything is launched; the vertical factor is unbounded.
 * Reference call site: DGP/models/eval.py:307-326. */
int  dgp_resize_crop_u8(const uint8_t* src, int32_t B, int32_t H, int32_t W, int32_t RH, int32_t RW, const int32_t* box, uint8_t* dst,
                        const int32_t* d_plan_x, const int32_t* d_plan_y, int32_t ksize_x, int32_t ksize_y, void* stream);

/* ---- The same resample with Pillow's other filters, over a window of one image (replaces crop_image + imresize (+ np.fliplr) of
 * the step-0 sample loader, PET/dataset/pose_defaultdataset.py:160-190 with PIL's BOX below scale 1 and BILINEAR above).  Filter ids
 * are Pillow's own constants.  Supports: BOX 0.5, BILINEAR 1, BICUBIC 2 (times filterscale); BOX is 1 on (-0.5, 0.5], BILINEAR is
 * 1 - |x| on (-1, 1).  BOX and BILINEAR evaluate the filter at (x + xmin - center + 0.5) * (1.0 / filterscale), Pillow's order;
 * BICUBIC keeps dgp_resize_plan's division, and its tables are dgp_resize_plan's integers. */
enum { DGP_FILTER_BILINEAR = 2, DGP_FILTER_BICUBIC = 3, DGP_FILTER_BOX = 4 };
/* Host only (no GPU): as dgp_resize_plan_size / dgp_resize_plan, for `filter`.  An unknown filter is DGP_ERR_INVALID. */
int  dgp_resize_plan_size_f(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize);
int  dgp_resize_plan_f(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, int32_t* coeffs);
/* src: ONE device uint8 image [src_H][src_W][3].  The inclusive window src[y0 .. y1][x0 .. x1] (0 <= x0 <= x1 < src_W, same for y) is
 * resampled to RH x RW with `filter`; mirror != 0 writes resized column c to column RW - 1 - c (np.fliplr after the resize).
 * dst: device uint8 [RH][RW][3].  d_plan_x ((x1 - x0 + 1) -> RW) and d_plan_y ((y1 - y0 + 1) -> RH): dgp_resize_plan_f's tables of
 * `filter`, laid out as for dgp_resize_crop_u8.  The window is addressed in place (origin + the image's row pitch): no copy is made,
 * and no byte outside the window's rows and columns reaches the result -- the tables are clamped to the window, and the dword-staged
 * bytes around a row segment are only ever multiplied by the zero padding of a table.  The LDS bound on the horizontal reduction is
 * dgp_resize_crop_u8's (DGP_ERR_INVALID before the launch).  Integer arithmetic, no atomics: the bytes are Pillow's. */
int  dgp_window_resize_u8(const uint8_t* src, int32_t src_H, int32_t src_W, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                          int32_t RH, int32_t RW, int32_t filter, int32_t mirror, uint8_t* dst, const int32_t* d_plan_x,
                          const int32_t* d_plan_y, int32_t ksize_x, int32_t ksize_y, void* stream);

/* ---- DLC target maps on the device (replaces compute_target_part_scoremap, PET/dataset/pose_defaultdataset.py:220-266, as called by
 * PoseDataset.make_batch for fit_dlc and by coord2map, DGP/dataset.py:246-271, for the DGP drivers).
 * entries: n_entries x (joint_id, x, y) doubles in the host function's person-then-joint order; offsets: int32 [n_frames + 1], frame f
 * owns entries [offsets[f], offsets[f + 1]).  Both are given twice: d_* on the device (read by the kernel) and h_* on the host, the
 * same values, checked before anything is launched: offsets[0] == 0 and non-decreasing, joint ids integral and in [0, nj), finite
 * coordinates, positive H, W, nj, n_frames, stride and locref_stdev (DGP_ERR_INVALID otherwise).
 * Outputs, fp32 on the device, any of them NULL: scmap [n][H][W][nj], weights [n][H][W][nj] (1 everywhere, or with
 * weigh_only_present_joints 1 in the channels of the frame's entries and 0 elsewhere), lmap and lmask [n][H][W][2 nj].  EVERY cell of
 * every given output is written (zeros included: no memset is needed, a frame without entries comes out zero).  A cell (y, x) takes
 * joint j's target from the LAST entry of j whose window holds it: cx = rint((x_j - stride / 2) / stride), the window is
 * [rint(max(cx - thr - 1, 0)), rint(min(cx + thr + 1, W - 1))] (skipped when empty), thr = pos_dist_thresh * scale, and the cell is
 * inside when dx^2 + dy^2 <= thr^2 with dx = x_j - (x stride + stride / 2); lmap = d * (1.0 / locref_stdev).  Double arithmetic without
 * contraction, cast to fp32 at the store: bit for bit the host function's values.  One thread per cell and joint group, no atomics. */
int  dgp_target_maps(const double* d_entries, const int32_t* d_offsets, const double* h_entries, const int32_t* h_offsets,
                     int32_t n_frames, int32_t H, int32_t W, int32_t nj, double stride, double pos_dist_thresh, double scale,
                     double locref_stdev, int32_t weigh_only_present_joints, float* scmap, float* weights, float* lmap, float* lmask,
                     void* stream);

/* ---- A DGP batch gathered on the device from frames kept there (replaces the per-iteration frame reads of Dataset.load_data,
 * DGP/dataset.py:811-821, and the host stack fed at fitdgp.py:762-764).
 * store: device uint8, n_slots frames at `store + slot * slot_stride`; slot_stride is in BYTES, a multiple of 16 and at least
 * frame_bytes (offsets are 64-bit: a store may pass 4 GiB).  patch: device uint8 [m][frame_bytes], packed: the frames uploaded for
 * this batch alone.  h_src: HOST int32 [nt]; output frame f is slot h_src[f] when h_src[f] >= 0 and patch frame -1 - h_src[f]
 * otherwise.  out: device uint8 [nt][frame_bytes], packed.  The table is checked here, before anything is launched (an entry at or
 * above n_slots or below -m, a bad pitch, a null pointer that would be read: DGP_ERR_INVALID), and reaches the kernel inside the
 * launch arguments, 64 frames per launch: no copy is issued and h_src may be reused as soon as the call returns.  nt == 0 launches
 * nothing.  A pure copy with plain vector loads and stores: 16 bytes per access when frame_bytes is a multiple of 16 and store, patch
 * and out are 16-byte aligned, single bytes otherwise.  store and patch may be NULL when n_slots / m is 0. */
int  dgp_gather_frames_u8(const uint8_t* store, int64_t n_slots, int64_t slot_stride, const uint8_t* patch, int32_t m,
                          const int32_t* h_src, int32_t nt, int64_t frame_bytes, uint8_t* out, void* stream);

/* ---- The augmenters of the DGP drivers' labeled frames on the device (replaces the pixel half of build_aug / data_aug,
 * DGP/models/fitdgp_util.py:412-451; host counterpart: deepgraphpose_amd/augment.py).  Every random number is drawn on the host; a
 * call gets the drawn parameters and ONE frame: src, dst device uint8 [H][W][3], packed, not overlapping, one launch on `stream`, one
 * thread per pixel, plain loads and stores.  Checked before the launch (DGP_ERR_INVALID): null pointers, H, W >= 2, a frame below
 * 2 GiB, src / dst overlap, finite parameters, table sizes that belong to (H, W).
 * affine: Pillow's Image.transform(AFFINE, BILINEAR) with the six HOST coefficients coef = (a, b, c, d, e, f): the sample position is
 *   (a (x + .5) + b (y + .5) + c, d (x + .5) + e (y + .5) + f) in double; 0 outside [0, W) x [0, H); else .5 off, floor, clamped
 *   neighbours, p0 + (p1 - p0) t along x then y (the row below replaced by the row itself past the edge), truncated.  Pillow's bytes.
 *   np.fliplr is coef = (-1, 0, W, 0, 1, 0), an exact permutation.
 * blur3: k = 3 x 3 HOST fp32 weights; out = rint(sum over (yy, xx) in that order of k[2 - yy][2 - xx] * src[y + yy - 1][x + xx - 1]),
 *   zero weights skipped, indices clamped to the frame, fp32 products and sums rounded one by one, clipped to [0, 255].
 * dropout: d_mask = DEVICE uint8 [h][w], 1 <= h <= H, 1 <= w <= W; pixel (y, x) is 0 where d_mask[min(y h / H, h - 1)][min(x w / W, w - 1)]
 *   is non-zero (integer division) and src elsewhere.
 * elastic: d_field = DEVICE fp32 [2][hc][wc] (dx, then dy), node (i, j) on pixel (4 i, 4 j), hc = ceil((H - 1) / 4) + 1 and wc alike;
 *   out[y][x] = bilinear sample of src, zeros outside, at (x + dx(y, x), y + dy(y, x)), d(y, x) the bilinear value of the coarse field
 *   at (y / 4, x / 4); fp32, rint, clipped.
 * noise: out = clip(rint(src + scale z)); z = Box-Muller over Philox4x32-10 with key (low, high half of `key`), counter (e / 4, 0, 0, 0),
 *   output word pair (0, 1) for e % 4 < 2 and (2, 3) otherwise, u = ((word >> 8) + 0.5) 2^-24, z = sqrt(-2 ln u_a) cos | sin (2 pi u_b)
 *   (cos for even e); e = (y W + x) 3 + c with per_channel, y W + x (one z for the three channels) without. */
int  dgp_aug_affine_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const double* coef, void* stream);
int  dgp_aug_blur3_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const float* k, void* stream);
int  dgp_aug_dropout_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const uint8_t* d_mask, int32_t h, int32_t w, void* stream);
int  dgp_aug_elastic_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, const float* d_field, int32_t hc, int32_t wc, void* stream);
int  dgp_aug_noise_u8(const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, float scale, int32_t per_channel, uint64_t key, void* stream);

/* ---- Baseline JPEG frames: entropy decode on the host, reconstruction on the device, Pillow's (libjpeg-turbo's) bytes (replaces the
 * decode half of moviepy's VideoFileClip for Motion-JPEG input, DGP/models/eval.py:256, and Pillow's per-frame decode of a directory of
 * JPEGs).  Accepted: SOF0 (baseline, 8-bit, Huffman), 1 or 3 components in ONE interleaved scan, luma sampling 1x1, 2x1 or 2x2 over
 * 1x1 chroma, 8-bit quantisation tables, YCbCr (JFIF, an Adobe APP14 marker with transform 1, or neither).  Everything else is
 * DGP_ERR_INVALID with the reason in dgp_last_error: progressive or arithmetic streams, 12-bit samples, 4 components, other
 * samplings, an Adobe transform that is not YCbCr, several scans, 16-bit tables, truncated or inconsistent segments.
 * Arithmetic: dequantise, libjpeg's "islow" inverse DCT (CONST_BITS 13, PASS1_BITS 2: columns first, descaled by 11 bits, then rows,
 * descaled by 18, + 128, clipped), "fancy" triangle upsampling of chroma on its true size ceil(H v / vmax) x ceil(W h / hmax) with
 * replicated edges (h2v1: (3 a + b + 1 | 2) >> 2; h2v2: column sums 3 a + b of the two nearest rows, then (3 s + t + 8 | 7) >> 4),
 * YCbCr -> RGB as y + ((FIX(1.402) cr + 32768) >> 16) etc. with FIX(x) = (int)(x 65536 + 0.5), clipped; grey is replicated. */
enum { DGP_JPEG_GRAY = 0, DGP_JPEG_444 = 1, DGP_JPEG_422 = 2, DGP_JPEG_420 = 3 };
typedef struct dgp_jpeg_info {
    int32_t width, height;
    int32_t ncomp;              /* 1 | 3 */
    int32_t sampling;           /* DGP_JPEG_* */
    int32_t mcus_x, mcus_y;     /* MCUs per row / column: 8 hmax x 8 vmax pixels each */
    int32_t blocks_x[3];        /* per component: blocks per row of its MCU-padded grid ... */
    int32_t blocks_y[3];        /* ... rows of blocks ... */
    int32_t blocks[3];          /* ... and their product */
    int32_t total_blocks;       /* sum over the components: a frame has total_blocks x 64 coefficients */
    int32_t restart_interval;   /* MCUs between RSTn markers, 0 = none */
    int32_t reserved;
    int64_t scan_offset;        /* offset of the first entropy-coded byte */
} dgp_jpeg_info;
/* Host only (no GPU), re-entrant: parses the marker segments of data[0 .. n) up to the scan header and fills *info. */
int    dgp_jpeg_probe(const uint8_t* data, int64_t n, dgp_jpeg_info* info);
/* Host only (no GPU), re-entrant, no globals, no allocation: any number of threads may decode at once.  info: dgp_jpeg_probe's of the
 * SAME stream (checked).  coef: int16 [total_blocks][64], the quantised coefficients de-zigzagged (natural order), planar by
 * component: all Y blocks row-major over the MCU-padded block grid, then Cb, then Cr.  qt: uint16 [ncomp][64], each component's table in
 * natural order.  DC prediction, EOB / ZRL, byte stuffing and DRI / RSTn follow T.81; Huffman table slots 0 and 1 that no DHT segment
 * defines get the typical tables of Annex K.3 (plain MJPEG frames carry none).  Every read is checked against n and every block address
 * against the geometry: a code that runs past 16 bits, a coefficient index past 63, data that ends early, a wrong restart marker or a
 * stream in which some |coefficient x table entry| exceeds 32767 (no encoder of 8-bit images writes one) is DGP_ERR_INVALID. */
int    dgp_jpeg_entropy_decode(const uint8_t* data, int64_t n, const dgp_jpeg_info* info, int16_t* coef, uint16_t* qt);
/* Host only: device scratch bytes dgp_jpeg_reconstruct_u8 needs for B frames (the component planes with their MCU padding); 0 for
 * arguments it would refuse. */
size_t dgp_jpeg_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t sampling);
/* d_coef: device int16 [B][total_blocks][64] and d_qt: device uint16 [B][ncomp][64] as dgp_jpeg_entropy_decode writes them, B frames
 * of ONE geometry (H, W, sampling), tables per frame.  dst: device uint8 [B][H][W][3] RGB, frames dst_frame_stride BYTES apart (at
 * least H W 3): a slice of a larger buffer is written in place and no byte between the frames is touched.  scratch: device,
 * 8-byte aligned, dgp_jpeg_scratch_bytes.  Two launches on `stream` (blocks -> planar uint8 in scratch; planes -> RGB), integer
 * arithmetic, no atomics: bit-identical from run to run, and Pillow's bytes.  B == 0 launches nothing. */
int    dgp_jpeg_reconstruct_u8(const int16_t* d_coef, const uint16_t* d_qt, int32_t B, int32_t H, int32_t W, int32_t sampling, uint8_t* dst,
                               int64_t dst_frame_stride, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Baseline JPEG frames, the other way: markers drawn and frames turned into quantised coefficients on the device, Huffman-coded on
 * the host, Pillow's (libjpeg-turbo's) bytes for save(quality=q, subsampling=s) of the drawn frame (replaces the draw + encode half of
 * the reference's annotated movie, DGP/models/eval.py:46-119).  Three components only: DGP_JPEG_444, _422 (h2v1) or _420; grey is
 * DGP_ERR_INVALID.  The coefficient buffer is the one dgp_jpeg_entropy_decode writes: the two halves are inverses on one format.
 * Arithmetic: Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16, Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16)
 * + 32767) >> 16, Cr alike, FIX(x) = (int)(x 65536 + 0.5); chroma downsampled without smoothing (h2v1: (a + b + bias) >> 1, bias 0, 1, 0,
 * 1 ... along the row; h2v2: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ...); edges replicated (pixel rows to a multiple of the vertical
 * factor, pixel columns to the component's real blocks, then the component's rows to its real blocks: ceil(ceil(W h / hmax) / 8) x
 * ceil(ceil(H v / vmax) / 8)); libjpeg's "islow" forward DCT on samples - 128 (CONST_BITS 13, PASS1_BITS 2: rows first, outputs 0 and 4
 * << 2, the rest descaled by 11; then columns, descaled by 2 and 15); quantised as sign(c) ((|c| + (8 q >> 1)) / (8 q)) with an exact
 * truncating divide.  Blocks of the MCU-padded grid beyond the real ones are dummy: AC 0, DC = the DC of the block before them in MCU
 * order (row-major inside the MCU), chains followed. */
/* Host only: libjpeg's tables for `quality` 1..100 (Annex K.1 / K.2 scaled by 5000 / q below 50, 200 - 2 q from there, (base scale + 50)
 * / 100 clamped to 1..255): qt uint16 [2][64], luminance then chrominance, natural order. */
int     dgp_jpeg_quality_tables(int32_t quality, uint16_t* qt);
/* Host only: bytes that always hold the stream of one H x W frame (header + every block at its worst case, stuffed); 0 for a geometry
 * the encoder refuses. */
int64_t dgp_jpeg_encode_bound(int32_t H, int32_t W, int32_t sampling);
/* Host only (no GPU), re-entrant, no globals, no allocation: any number of threads may encode at once.  coef: int16 [total_blocks][64]
 * (natural order, planar by component, row-major over the MCU-padded grid), qt: uint16 [2][64], entries 1..255.  Writes into out[0 .. cap)
 * the complete stream: SOI, JFIF APP0 (1.01, units 0, density 1 x 1), DQT 0, DQT 1, SOF0, DHT DC0 / AC0 / DC1 / AC1 (Annex K.3), SOS,
 * the entropy-coded data with byte stuffing and the last byte padded with 1-bits, EOI; no restart markers.  *n = its length.
 * DGP_ERR_INVALID with the reason in dgp_last_error for a stream that would pass cap (nothing is written at or past out + cap), a DC
 * difference beyond category 11 or an AC coefficient beyond category 10, a table entry outside 1..255, a bad geometry. */
int     dgp_jpeg_entropy_encode(const int16_t* coef, int32_t H, int32_t W, int32_t sampling, const uint16_t* qt, uint8_t* out, int64_t cap,
                                int64_t* n);
/* Host only: device scratch bytes dgp_jpeg_forward_u8 needs for B frames (the padded component planes); 0 for arguments it refuses. */
size_t  dgp_jpeg_forward_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t sampling);
/* src: device uint8 [B][H][W][3] RGB, frames src_frame_stride BYTES apart (at least H W 3): a slice of a larger buffer is read in place,
 * and src is never written.  d_qt: device uint16 [2][64], one table pair per call.  d_markers: null, or device int32 [B][n_markers][6] =
 * row, col, r, g, b, on: a pixel inside [row - dotsize, row + dotsize] x [col - dotsize, col + dotsize] of a marker with on != 0 takes
 * that marker's colour before the conversion, the highest marker index that covers it wins, squares are clipped to the frame.  The
 * overlay happens in registers while the pixels are read: no pass over the frames of its own.  d_coef: device int16
 * [B][total_blocks][64], 16-byte aligned.  scratch: device, 8-byte aligned, dgp_jpeg_forward_scratch_bytes.  Two launches on `stream`
 * (pixels -> padded component planes in scratch; planes -> blocks), integer arithmetic, no atomics: bit-identical from run to run.
 * B == 0 launches nothing. */
int     dgp_jpeg_forward_u8(const uint8_t* src, int32_t B, int32_t H, int32_t W, int64_t src_frame_stride, int32_t sampling,
                            const uint16_t* d_qt, const int32_t* d_markers, int32_t n_markers, int32_t dotsize, int16_t* d_coef,
                            void* scratch, size_t scratch_bytes, void* stream);

/* ---- Frame selection: thumbnails and k-means on the device (replaces the per-frame resize and the clustering of
 * KmeansbasedFrameselection / KmeansbasedFrameselectioncv2, deeplabcut/utils/frameselectiontools.py:139-246, used by extract_frames and
 * by extract_outlier_frames' ExtractFramesbasedonPreselection).  No float atomics anywhere: the same input gives the same bits.
 *
 * Thumbnails, exact integer area averages.  frames: device uint8, N frames of [H][W][3], frame_stride BYTES apart (at least H W 3), at
 * ANY byte address.  The window frame[y1:y2, x1:x2] (0 <= x1 < x2 <= W, same for y; Hc = y2 - y1, Wc = x2 - x1) is reduced to oh x ow
 * values: column box i is [floor(i Wc / ow), floor((i + 1) Wc / ow)), rows alike with oh, and oh MUST be max(1, Hc ow / Wc rounded half
 * to even) -- the caller states it, it is checked.  ow > Wc (an upsample) is DGP_ERR_INVALID.  color == 0: one value per box, the integer
 * sum over the box's pixels and three channels / (pixels x 3), out row = [oh][ow]; color != 0: one value per channel, out row =
 * [oh][3][ow] (the reference's hstack of the three planes).  A value is (float)((double)sum / (double)count), nothing else.  out: device
 * fp32, row f at out + f out_stride (FLOATS, at least D = oh ow (1 | 3)); only the D values of each row are written.
 * Limits (DGP_ERR_INVALID before anything is launched): Wc <= 16384, ow <= 1024, and the largest box (ceil(Wc / ow) x ceil(Hc / oh)
 * pixels) x 3 x 255 must fit 32 bits (5 614 429 pixels), so an all-255 frame cannot overflow a counter.
 * One workgroup per (frame, output row); 16-byte loads when the address of every row allows it (frames, frame_stride and 3 W multiples
 * of 16), 4-byte loads likewise, single bytes otherwise; per-column integer counters in LDS (integer LDS atomics: order-independent). */
int  dgp_frame_features_u8(const uint8_t* frames, int32_t N, int32_t H, int32_t W, int64_t frame_stride, int32_t x1, int32_t x2,
                           int32_t y1, int32_t y2, int32_t ow, int32_t oh, int32_t color, float* out, int64_t out_stride, void* stream);

/* Limits of the three k-means entry points: 1 <= k <= DGP_KMEANS_MAX_K, 1 <= D <= DGP_KMEANS_MAX_D (30 x 30 x 3 thumbnails are 2700),
 * 1 <= N, N D < 2^31.  Rows are grouped in slabs: S = min(DGP_KMEANS_MAX_SLABS, ceil(N / 256)) slabs of ceil(N / S) rows (the last one
 * shorter); a column sum is one double accumulator per slab walked in row order, and the slabs are added in slab order. */
enum { DGP_KMEANS_MAX_K = 160, DGP_KMEANS_MAX_D = 8192, DGP_KMEANS_MAX_SLABS = 64 };
/* Host only: device scratch bytes dgp_kmeans_center (k = 0) or dgp_kmeans_update needs; 0 for arguments they refuse. */
size_t dgp_kmeans_scratch_bytes(int64_t N, int32_t D, int32_t k);
/* X: device fp32 [N][D], packed.  mean[d] = (float)(column sum / N) (DATA.mean(axis=0), :231), then X[r][d] = X[r][d] - mean[d] in fp32,
 * in place.  mean: device fp32 [D].  scratch: device, 8-byte aligned, dgp_kmeans_scratch_bytes(N, D, 0).  Three launches. */
int  dgp_kmeans_center(float* X, int64_t N, int32_t D, float* mean, void* scratch, size_t scratch_bytes, void* stream);
/* Nearest centre of every row.  C: device fp32 [k][D].  labels: device int32 [N], read (the previous labels, any values) and
 * overwritten; dist: device fp32 [N], the squared distance to the chosen centre; changed: device int32, set to the number of rows whose
 * label differs from the one that was there (an integer counter: exact).  Distances are the direct form sum_d (x_d - c_d)^2 in fp32,
 * every product and sum rounded on its own, in a FIXED order: D is cut into chunks of DC = min(512, floor(10240 / k) rounded down to a
 * multiple of 64) columns; inside a chunk lane l of a 64-lane wave adds its columns l, l + 64, ... in that order (columns past D count
 * as zero), the 64 partial sums are combined by a butterfly (v += v of lane ^ 32, ^ 16, ... ^ 1), and the chunk totals are added in
 * chunk order.  On an exact tie the lowest centre index wins.  One wave per row, the centres of a chunk staged in LDS (40 KB), the
 * running sums of a workgroup's 32 rows in LDS as well. */
int  dgp_kmeans_assign(const float* X, int64_t N, int32_t D, const float* C, int32_t k, int32_t* labels, float* dist, int32_t* changed,
                       void* stream);
/* Every centre becomes the mean of its members: (float)(sum / count), the sum as described above (members only, in row order).  An
 * empty cluster keeps its centre and gets count 0.  counts: device int32 [k + 1]; counts[k] is the number of labels outside [0, k):
 * such a row indexes nothing, it is skipped and counted.  scratch: dgp_kmeans_scratch_bytes(N, D, k).  Two launches. */
int  dgp_kmeans_update(const float* X, int64_t N, int32_t D, const int32_t* labels, float* C, int32_t k, int32_t* counts, void* scratch,
                       size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DGP_HIP_H */
