// Optimisers of the training step over the trainer's flat buffers: global-norm clip + momentum SGD (clip_by_global_norm(10),
// MomentumOptimizer(0.9)) or Adam, host <-> device copies of the buffers, and the one-synchronisation step status.
#include "dgp_train.h"

using namespace dgp;

namespace {

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long long n, double* __restrict__ out) {
    __shared__ double part[4];
    double s = 0.0;
    const long long n4 = n >> 2;                 // 16-byte loads (hipMalloc'ed buffer), the tail one by one
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = g4[i];
        s += (double)v.x * (double)v.x + (double)v.y * (double)v.y + (double)v.z * (double)v.z + (double)v.w * (double)v.w;
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        s += (double)g[i] * (double)g[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

__global__ void momentum_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ v, long long n,
                                float lr, float mom, float clip, const double* __restrict__ sumsq, double* __restrict__ sumsq_next,
                                float* __restrict__ gnorm_out, const int* __restrict__ skip) {
    // skip: the range flag of a 16-bit / fast pass -- set: that pass's gradients are invalid, nothing is updated (the host repeats the step)
    // sumsq_next: the accumulator the NEXT step's sumsq_kernel adds into (nobody reads it now): zeroed here instead of by a fill launch
    const float gn = (float)sqrt(*sumsq);
    if (blockIdx.x == 0 && threadIdx.x == 0) *sumsq_next = 0.0;
    if (skip && *skip) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && gnorm_out) *gnorm_out = gn;
        return;
    }
    const float scale = clip > 0.f ? clip / fmaxf(gn, clip) : 1.f;      // tf.clip_by_global_norm; clip <= 0: none
    if (blockIdx.x == 0 && threadIdx.x == 0 && gnorm_out) *gnorm_out = gn;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float a = mom * v[i] + g[i] * scale;            // accum = momentum * accum + grad
        v[i] = a;
        w[i] -= lr * a;                                       // var -= lr * accum
    }
}

// tf.train.AdamOptimizer's dense update (ApplyAdam, fp32) behind tf.clip_by_global_norm, one stream over four arrays: per parameter it
// reads w, g, m, v and writes w, m, v (28 bytes; sumsq_kernel read g once before: 32 in all).  16-byte accesses (hipMalloc'ed buffers),
// the last n % 4 elements one by one.  pow_cur = {beta1^t, beta2^t} of THIS step (t = applied steps + 1), read by every workgroup;
// pow_next is the other half of the ping-pong pair (nobody reads it now): thread 0 writes cur * beta into it, or cur itself when the
// step is skipped -- the host flips the index per call either way and never learns whether the step was applied.
__device__ __forceinline__ void adam_one(float& w, float g, float& m, float& v, float scale, float alpha, float omb1, float beta2, float omb2, float eps) {
    const float gs = g * scale;
    m += (gs - m) * omb1;                                     // m += (g - m) (1 - beta1)
    // v += (g g - v) (1 - beta2), written as the convex combination it is: a second moment that overflowed to +inf (g g beyond fp32)
    // stays +inf -- the step size stays 0 -- where the incremental form would turn it into inf - inf
    v = beta2 * v + omb2 * (gs * gs);
    w -= (m * alpha) / (sqrtf(v) + eps);                      // var -= (m alpha) / (sqrt(v) + eps), the grouping of TF's functor
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   long long n, float lr, float beta1, float beta2, float eps, float clip,
                                                   const double* __restrict__ sumsq, double* __restrict__ sumsq_next,
                                                   const float* __restrict__ pow_cur, float* __restrict__ pow_next,
                                                   float* __restrict__ gnorm_out, const int* __restrict__ skip) {
    const float gn = (float)sqrt(*sumsq);
    const float b1p = pow_cur[0], b2p = pow_cur[1];
    const bool skipped = skip && *skip;                       // (see momentum_kernel)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *sumsq_next = 0.0;
        if (gnorm_out) *gnorm_out = gn;
        pow_next[0] = skipped ? b1p : b1p * beta1;
        pow_next[1] = skipped ? b2p : b2p * beta2;
    }
    if (skipped) return;
    const float scale = clip > 0.f ? clip / fmaxf(gn, clip) : 1.f;      // tf.clip_by_global_norm; clip <= 0: none
    const float alpha = lr * sqrtf(1.f - b2p) / (1.f - b1p);
    const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
    const long long n4 = n >> 2;
    float4* w4 = reinterpret_cast<float4*>(w);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 ww = w4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        adam_one(ww.x, gg.x, mm.x, vv.x, scale, alpha, omb1, beta2, omb2, eps);
        adam_one(ww.y, gg.y, mm.y, vv.y, scale, alpha, omb1, beta2, omb2, eps);
        adam_one(ww.z, gg.z, mm.z, vv.z, scale, alpha, omb1, beta2, omb2, eps);
        adam_one(ww.w, gg.w, mm.w, vv.w, scale, alpha, omb1, beta2, omb2, eps);
        m4[i] = mm; v4[i] = vv; w4[i] = ww;
    }
    for (long long i = 4 * n4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        adam_one(w[i], g[i], m[i], v[i], scale, alpha, omb1, beta2, omb2, eps);
}

__global__ void step_status_kernel(const float* __restrict__ losses, int n_losses, const float* __restrict__ gnorm, const int* __restrict__ flag,
                                   float* __restrict__ host) {
    const int t = threadIdx.x;
    if (t < n_losses) host[t] = losses[t];
    if (t == 8) host[8] = *gnorm;
    if (t == 9) host[9] = flag ? (float)*flag : 0.f;
    __threadfence_system();
}

}  // namespace

// Adam's slots on first use: m = v = 0, both power pairs {beta1, beta2} (TF's non-slot variables start there)
static int adam_alloc(dgp_trainer* tr, float beta1, float beta2) {
    if (tr->adam_m) return DGP_OK;
    const size_t nb = (size_t)tr->n_train * sizeof(float);
    float *m = nullptr, *v = nullptr, *p = nullptr;
    const float pw[4] = {beta1, beta2, beta1, beta2};
    if (hipMalloc(&m, nb) != hipSuccess || hipMalloc(&v, nb) != hipSuccess || hipMalloc(&p, sizeof(pw)) != hipSuccess ||
        hipMemset(m, 0, nb) != hipSuccess || hipMemset(v, 0, nb) != hipSuccess ||
        hipMemcpy(p, pw, sizeof(pw), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {                 // (once: the fills are done before a kernel on any stream reads the slots)
        for (float* q : {m, v, p}) if (q) (void)hipFree(q);
        return fail(DGP_ERR_HIP, "dgp_adam_clip: hipMalloc of the Adam slots failed");
    }
    tr->adam_m = m; tr->adam_v = v; tr->d_adam_pow = p; tr->adam_pow_k = 0;
    return DGP_OK;
}

// floats behind dgp_trainer_buffer(tr, 5 .. 7): a copy must stay inside them
static long long buffer_floats(const dgp_trainer* tr, int32_t which) { return which == 7 ? 2 : tr->n_train; }

extern "C" {

/* host <-> device copies of a slice of one of the flat buffers (which: 0 params, 1 grads, 2 momentum, 3 stats, 5 / 6 Adam's m / v, 7 its two
 * powers; an upload into 5 - 7 allocates Adam's slots, a download from them before that fails) */
int dgp_trainer_upload(dgp_trainer* tr, int32_t which, int64_t offset, const float* host, int64_t n) {
    if (tr && which >= 5 && which <= 7 && adam_alloc(tr, 0.9f, 0.999f) != DGP_OK) return DGP_ERR_HIP;
    float* b = dgp_trainer_buffer(tr, which);
    if (!b || !host || offset < 0 || n < 0) return fail(DGP_ERR_INVALID, "dgp_trainer_upload: bad argument");
    if (which >= 5 && offset + n > buffer_floats(tr, which)) return fail(DGP_ERR_INVALID, "dgp_trainer_upload: past the end of the buffer");
    if (which >= 5) HIP_TRY(hipDeviceSynchronize());          // (the slots may be in use by an optimiser step still in flight)
    HIP_TRY(hipMemcpy(b + offset, host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return DGP_OK;
}
int dgp_trainer_download(dgp_trainer* tr, int32_t which, int64_t offset, float* host, int64_t n) {
    float* b = dgp_trainer_buffer(tr, which);
    if (!b || !host || offset < 0 || n < 0) return fail(DGP_ERR_INVALID, "dgp_trainer_download: bad argument");
    if (which >= 5 && offset + n > buffer_floats(tr, which)) return fail(DGP_ERR_INVALID, "dgp_trainer_download: past the end of the buffer");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, b + offset, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return DGP_OK;
}

int dgp_sgd_momentum_clip(dgp_trainer* tr, float lr, float momentum, float clip_norm, float* gnorm_host_or_null, void* stream) {
    if (!tr) return fail(DGP_ERR_INVALID, "dgp_sgd_momentum_clip: null");
    hipStream_t s = (hipStream_t)stream;
    const int k = tr->sumsq_k;
    tr->sumsq_k ^= 1;
    // (768 workgroups, three per CU: every workgroup ends in ONE fp64 atomic on the same address, and 4 096 of them in a row cost more than the 102 MB read)
    const int sumsq_grid = grid_for(tr->n_train) < 768 ? grid_for(tr->n_train) : 768;
    hipLaunchKernelGGL(sumsq_kernel, dim3(sumsq_grid), dim3(256), 0, s, tr->grads, tr->n_train, tr->d_sumsq + k);
    hipLaunchKernelGGL(momentum_kernel, dim3(grid_for(tr->n_train)), dim3(256), 0, s, tr->params, tr->grads, tr->mom, tr->n_train,
                       lr, momentum, clip_norm, tr->d_sumsq + k, tr->d_sumsq + (k ^ 1), tr->d_gnorm, tr->fwd_fast ? tr->d_fast_flag : nullptr);
    HIP_TRY(hipGetLastError());
    if (gnorm_host_or_null) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(gnorm_host_or_null, tr->d_gnorm, sizeof(float), hipMemcpyDeviceToHost));
    }
    return DGP_OK;
}

/* tf.clip_by_global_norm(clip_norm) + tf.train.AdamOptimizer's dense update; same contract as dgp_sgd_momentum_clip.  The powers advance
 * on the device, and only when the step is applied (adam_kernel) */
int dgp_adam_clip(dgp_trainer* tr, float lr, float beta1, float beta2, float eps, float clip_norm, float* gnorm_host_or_null, void* stream) {
    if (!tr) return fail(DGP_ERR_INVALID, "dgp_adam_clip: null");
    if (adam_alloc(tr, beta1, beta2) != DGP_OK) return DGP_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const int k = tr->sumsq_k, pk = tr->adam_pow_k;
    tr->sumsq_k ^= 1;
    tr->adam_pow_k ^= 1;
    const int sumsq_grid = grid_for(tr->n_train) < 768 ? grid_for(tr->n_train) : 768;      // (see dgp_sgd_momentum_clip)
    hipLaunchKernelGGL(sumsq_kernel, dim3(sumsq_grid), dim3(256), 0, s, tr->grads, tr->n_train, tr->d_sumsq + k);
    // a grid-stride stream: 2 048 workgroups of 256 (eight per CU), each thread four parameters per trip
    const int grid = grid_for((tr->n_train + 3) / 4) < 2048 ? grid_for((tr->n_train + 3) / 4) : 2048;
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, s, tr->params, tr->grads, tr->adam_m, tr->adam_v, tr->n_train,
                       lr, beta1, beta2, eps, clip_norm, tr->d_sumsq + k, tr->d_sumsq + (k ^ 1), tr->d_adam_pow + 2 * pk,
                       tr->d_adam_pow + 2 * (pk ^ 1), tr->d_gnorm, tr->fwd_fast ? tr->d_fast_flag : nullptr);
    HIP_TRY(hipGetLastError());
    if (gnorm_host_or_null) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(gnorm_host_or_null, tr->d_gnorm, sizeof(float), hipMemcpyDeviceToHost));
    }
    return DGP_OK;
}

/* One synchronisation for a whole step enqueued without read-backs (forward, loss, backward, dgp_sgd_momentum_clip with a NULL
 * gnorm pointer, dgp_trainer_sync_weights): waits for the device, then *gnorm = the global gradient norm the optimiser saw and the
 * fast / 16-bit pass status as dgp_trainer_fast_status reports it.  When *failed != 0 the optimiser skipped its update on the device
 * (the flag is read by the momentum kernel), so the step can simply be run again on the parity path. */
int dgp_trainer_step_status(dgp_trainer* tr, const float* d_losses, int32_t n_losses, float* losses, float* gnorm, int32_t* was_fast,
                            int32_t* failed, void* stream) {
    if (!tr) return fail(DGP_ERR_INVALID, "dgp_trainer_step_status: null");
    if (n_losses < 0 || n_losses > 8 || (n_losses && (!d_losses || !losses))) return fail(DGP_ERR_INVALID, "dgp_trainer_step_status: 0..8 losses");
    hipStream_t s = (hipStream_t)stream;
    // one tiny kernel at the end of the stream writes everything the host wants into pinned memory; one wait.  (Every launch of the step
    // is on this stream or joined into it: the second stream's forward chain and weight gradients, the optimiser, the re-packing.)
    hipLaunchKernelGGL(step_status_kernel, dim3(1), dim3(64), 0, s, d_losses, n_losses, tr->d_gnorm, tr->fwd_fast ? tr->d_fast_flag : (const int*)nullptr,
                       tr->h_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n_losses; ++i) losses[i] = tr->h_status[i];
    if (gnorm) *gnorm = tr->h_status[8];
    if (was_fast) *was_fast = tr->fwd_fast ? 1 : 0;
    if (failed) *failed = (int32_t)tr->h_status[9];
    return DGP_OK;
}

}  // extern "C"
